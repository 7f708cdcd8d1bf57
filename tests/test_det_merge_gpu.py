"""Sharded dataset inference on the GPU (u3d_det_store_merge, det_store.gather_stores, testing.ShardPlan): the merge bit for bit against
the NumPy restatement of tests/det_merge_ref.py into a poisoned store that already holds scenes, more than one step of every loop,
every refusal, the argument checks, no host synchronisation; gather_stores in two and three processes over gloo on one GPU (and over
RCCL where two GPUs exist) against the one-store statement, a failing rank that must not hang its peer, and test_dataset sharded over
two processes against the one-process loop.

Every comparison here is equality: a merge only copies."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import det_merge_ref as mref
import det_store_ref as ref
from test_det_store_gpu import SEED, _assert_store, _buffers, _det, _poisoned, _same_dict, _store_loop, _World
from test_dist_gpu import _free_port
from test_varlen_gpu import _no_host_sync
from uni3detr_amd import native as nv
from uni3detr_amd import testing
from uni3detr_amd.det_store import DetStore, gather_stores
from uni3detr_amd.testing import ShardPlan

pytestmark = pytest.mark.gpu
K = 5


def _up(arrays, cuda):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _shards(rng, plan, k, D, full=(), big=None):
    """the RefStores of a plan's ranks: every scene with a random count in [0, k], the positions in `full` with k, `big` = (position,
    count) with a count of its own"""
    W, B = plan.world, plan.batch_size
    most = max(k, big[1] if big else 0)
    stores = [ref.RefStore(max(plan.scenes(r), 1), max(plan.scenes(r), 1) * most, D, 0) for r in range(W)]
    for j in range(plan.n_batches):
        pos = list(range(j * B, min((j + 1) * B, plan.n_scenes)))
        counts = [big[1] if big and p == big[0] else k if p in full else int(rng.integers(0, k + 1)) for p in pos]
        assert stores[j % W].append(*ref.random_det(rng, len(pos), most, D, counts=counts))
    return stores


def _both(st, want, w, m, cuda):
    """the same merge on the device store and on the restatement -> accepted?"""
    t = _up(w, cuda)
    nv.det_store_merge(*t, torch.from_numpy(m).to(cuda), st.boxes, st.scores, st.labels, st.table, st.cursor, st.invalid)
    return mref.merge(want, *w, m)


def _with_two_scenes(cuda, S, D, R, rng):
    """a poisoned store (and its restatement) that already holds two scenes"""
    st, want = _poisoned(cuda, S, D, R=R, M=2)
    early = ref.random_det(rng, 2, K, D, counts=[3, 0])
    st.append(_det(early, cuda))
    assert want.append(*early)
    return st, want


# ---- 1: the contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [7, 9])
def test_merge_matches_restatement(cuda, D):
    rng = np.random.default_rng(D)
    plan = ShardPlan(4, 2, 3)                                                # two batches over three ranks: shard 2 is empty
    assert plan.scenes(2) == 0
    stores = _shards(rng, plan, K, D, full=(1,))
    stores[1].table[0, 1] = 0                                                 # counts 0 and K both present (scene 2 emptied in its shard)
    w = mref.wire(stores, Nmax=2 * K + 3, Smax=3, pad_f=np.nan, pad_i=ref.POISON_I)      # padding past every shard's own part
    counts = np.concatenate([np.diff(w[3][r, :w[4][r, 0] + 1]) for r in (0, 1)])
    assert 0 in counts and K in counts and w[4].tolist()[2] == [0, 0]
    st, want = _with_two_scenes(cuda, 9, D, 40, rng)
    assert _both(st, want, w, plan.scene_map(), cuda)
    _assert_store(st, want)                                                   # every buffer, poison included
    assert want.cursor.tolist() == [6, 3 + int(w[4][:, 1].sum()), 0, 0]
    # a second merge appends behind the first; a map entry named twice is copied twice, in map order
    m2 = np.array([[1, 1], [0, 0], [1, 1]], np.int32)
    assert _both(st, want, w, m2, cuda)
    _assert_store(st, want)
    assert len(st) == 9 and st.invalid_batches() == []
    got = st.packed(3)
    for name, g, x in zip(("boxes", "scores", "labels", "off"), got, want.pack()[:4]):
        assert np.array_equal(g.cpu().numpy(), x), name


def test_offsets_are_read_clamped(cuda):
    rng = np.random.default_rng(11)
    plan = ShardPlan(6, 2, 2)
    w = list(mref.wire(_shards(rng, plan, K, 7, full=(0, 1, 4, 5)), pad_f=np.nan, pad_i=ref.POISON_I))
    w[3] = w[3].copy()
    w[3][0, 1], w[3][0, 3], w[3][1, 2] = -5, int(w[4][0, 1]) + 9, 2 ** 31 - 1       # below 0, past the shard's rows, far past them
    st, want = _with_two_scenes(cuda, 8, 7, 6 * K + 3, rng)
    assert _both(st, want, w, plan.scene_map(), cuda)
    _assert_store(st, want)
    assert not np.isnan(want.boxes[:want.cursor[1]]).any()                    # no padding row came along


# ---- 2: more than one step of every loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, W", [(130, 3), (600, 260)])
def test_more_than_one_step_of_every_loop(cuda, n, W):
    """130 scenes: three steps of a 64-lane scan, every wave of the plan's workgroup with its own total; 600 scenes over 260 shards: three
    steps of the plan's 256 scenes, the last one partial, and two of its head loop.  Scene 77 holds 40 rows: 280 dwords, past one
    256-thread stride of the copy."""
    rng = np.random.default_rng(n)
    plan = ShardPlan(n, 1, W)
    w = mref.wire(_shards(rng, plan, 3, 7, big=(77, 40)), pad_f=np.nan, pad_i=ref.POISON_I)
    rows = int(w[4][:, 1].sum())
    st, want = _with_two_scenes(cuda, n + 2, 7, rows + 3, rng)                # room for exactly this merge
    bad = plan.scene_map()
    bad[n - 1, 1] += 1                                                        # a bad entry in the last step refuses the call
    assert not _both(st, want, w, bad, cuda)
    _assert_store(st, want)
    assert _both(st, want, w, plan.scene_map(), cuda)
    _assert_store(st, want)
    assert want.cursor.tolist() == [n + 2, rows + 3, 0, 1] and want.table[2 + 77, 1] == 40


# ---- 3: refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["scenes", "rows", "shard", "shard_negative", "local", "head_scenes", "head_rows", "cursor"])
def test_a_refused_merge_writes_nothing(cuda, what):
    rng = np.random.default_rng(5)
    plan = ShardPlan(6, 2, 2)
    w = list(mref.wire(_shards(rng, plan, K, 7, full=(0,)), pad_f=np.nan, pad_i=ref.POISON_I))
    m = plan.scene_map()
    rows = int(w[4][:, 1].sum())
    S, R = (7 if what == "scenes" else 8), (rows + 2 if what == "rows" else rows + 3)
    st, want = _with_two_scenes(cuda, S, 7, R, rng)
    if what in ("shard", "shard_negative"):
        m[3, 0] = 2 if what == "shard" else -1
    if what == "local":
        m[4, 1] = int(w[4][m[4, 0], 0])
    if what.startswith("head"):
        w[4] = w[4].copy()
        w[4][1] = (w[3].shape[1], 0) if what == "head_scenes" else (0, w[0].shape[1] + 1)       # shard 1 is not even named by the map
        m = m[m[:, 0] == 0]
    if what == "cursor":
        st.cursor[0], want.cursor[0] = 9, 9
    before = _buffers(st)
    assert not _both(st, want, w, m, cuda)
    after = _buffers(st)
    for k in ("boxes", "scores", "labels", "table", "invalid"):
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    assert after["cursor"].tolist() == before["cursor"][:3].tolist() + [1]
    _assert_store(st, want)
    if what != "cursor":                                                      # the same store takes what does fit
        ok = ref.random_det(rng, 1, K, 7, counts=[1])
        st.append(_det(ok, cuda))
        assert want.append(*ok)
        _assert_store(st, want)


def test_an_empty_map_validates_and_moves_nothing(cuda):
    rng = np.random.default_rng(6)
    w = list(mref.wire(_shards(rng, ShardPlan(4, 2, 2), K, 7)))
    st, want = _with_two_scenes(cuda, 4, 7, 20, rng)
    none = np.zeros((0, 2), np.int32)
    assert _both(st, want, w, none, cuda)
    _assert_store(st, want)
    w[4] = w[4].copy()
    w[4][0, 1] = -1
    assert not _both(st, want, w, none, cuda)
    _assert_store(st, want)
    assert want.cursor.tolist() == [2, 3, 0, 1]


# ---- 4: bad arguments, no host synchronisation ------------------------------------------------------------------------------------
def test_merge_refuses_bad_arguments(cuda):
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=cuda)                 # noqa: E731
    i32, p = torch.int32, nv._ptr
    sh = [z(2, 5, 7), z(2, 5), z(2, 5, dt=i32), z(2, 4, dt=i32), z(2, 2, dt=i32)]
    m = z(3, 2, dt=i32)
    st = [z(16, 7), z(16), z(16, dt=i32), z(4, 2, dt=i32), z(4, dt=i32)]
    ws = z(64, dt=i32)

    def call(W=2, Nmax=5, Smax=3, D=7, n=3, R=16, S=4, boxes=True, work=256):
        return nv.lib().u3d_det_store_merge(p(sh[0]) if boxes else None, *[p(t) for t in sh[1:]], W, Nmax, Smax, D, p(m), n,
                                            *[p(t) for t in st], None, R, S, 0, p(ws), work, nv._stream())

    assert call(D=8) == -1 and call(W=0) == -1 and call(Nmax=0) == -1 and call(n=-1) == -1 and call(Smax=-1) == -1
    assert call(R=0) == -1 and call(S=0) == -1 and call(boxes=False) == -1
    assert call(R=2 ** 31 // 7 + 1) == nv.U3D_ERR_UNSUPPORTED and call(W=2 ** 10, Nmax=2 ** 19) == nv.U3D_ERR_UNSUPPORTED
    assert call(work=nv.det_store_merge_workspace(3) - 1) == -4
    torch.cuda.synchronize()
    assert all(not bool(t.any()) for t in st + [ws])                          # nothing was launched
    sh[4][:, 0] = 3
    assert call() == 0                                                        # (the call itself is a good one: three empty scenes)
    torch.cuda.synchronize()
    assert st[4].tolist() == [3, 0, 0, 0]


def test_merge_runs_without_host_sync(cuda):
    rng = np.random.default_rng(7)
    plan = ShardPlan(5, 2, 2)
    w = mref.wire(_shards(rng, plan, K, 7))
    t, m = _up(w, cuda), torch.from_numpy(plan.scene_map()).to(cuda)
    st, want = _poisoned(cuda, 10, 7, R=60, M=0)
    ws = torch.empty((nv.det_store_merge_workspace(5),), dtype=torch.uint8, device=cuda)
    nv.det_store_merge(*t, m, st.boxes, st.scores, st.labels, st.table, st.cursor, st.invalid, workspace=ws)      # (the code object loads)
    torch.cuda.synchronize()
    with _no_host_sync():
        nv.det_store_merge(*t, m, st.boxes, st.scores, st.labels, st.table, st.cursor, st.invalid, workspace=ws)
        nv.det_store_merge(*t, m[:0], st.boxes, st.scores, st.labels, st.table, st.cursor, st.invalid)            # allocates its own
    torch.cuda.synchronize()
    for _ in range(2):
        assert mref.merge(want, *w, plan.scene_map())
    _assert_store(st, want)


def test_gather_stores_alone_is_the_same_path(cuda):
    """no process group: world 1, no collectives - the store comes back as a copy in dataset order, and a bad store raises"""
    rng = np.random.default_rng(8)
    st, want = _poisoned(cuda, 6, 7, M=2)
    for _ in range(2):
        arrays = ref.random_det(rng, 3, K, 7)
        st.append(_det(arrays, cuda))
        want.append(*arrays)
    assert not dist.is_initialized()
    whole = gather_stores(st, ShardPlan(6, 3, 1), num_classes=3)
    assert whole is not st and len(whole) == 6 and whole.invalid_batches() == [] and whole.row_capacity == max(int(want.cursor[1]), 1)
    for g, x in zip(whole.packed(3), want.pack()[:4]):
        assert np.array_equal(g.cpu().numpy(), x)
    with pytest.raises(RuntimeError, match="rank 0 of 1.*holds 6 scenes, the plan gives it 5"):
        gather_stores(st, ShardPlan(5, 3, 1))
    with pytest.raises(ValueError, match="rank 0 of 1: DetStore: labels must lie in \\[0, 1\\)"):
        gather_stores(st, ShardPlan(6, 3, 1), num_classes=1)
    with pytest.raises(ValueError, match="plan for 2 rank"):
        gather_stores(st, ShardPlan(6, 3, 2))
    st.append(_det(ref.random_det(rng, 3, K, 7), cuda))                       # 9 scenes into 6
    with pytest.raises(RuntimeError, match="rank 0 of 1.*refused"):
        gather_stores(st, ShardPlan(6, 3, 1))


# ---- 5: several processes -----------------------------------------------------------------------------------------------------------
def _global_batch(j, B, D):
    return ref.random_det(np.random.default_rng(1000 + j), B, K, D)         # counts 0 and K in every batch


def _one_store_statement(n, B, D):
    per_scene = []
    for j in range(-(-n // B)):
        b, s, l, c = _global_batch(j, B, D)
        per_scene += [(b[i, :c[i]], s[i, :c[i]], l[i, :c[i]]) for i in range(min((j + 1) * B, n) - j * B)]
    return ref.concat_lists(per_scene, D)


def _gather_worker(rank, world, port, q, backend, rounds):
    """rounds: [(n scenes, B, rank whose last append is left invalid or None), ...] - one gather_stores each, in one process group"""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dev = torch.device("cuda", rank if backend == "nccl" else 0)
        torch.cuda.set_device(dev)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        out = []
        for n, B, failing in rounds:
            plan = ShardPlan(n, B, world)
            store = DetStore(max(plan.scenes(rank), 1), K, 7, dev)
            ids = plan.batch_ids(rank)
            for j in ids:
                live = torch.tensor([min((j + 1) * B, n) - j * B], dtype=torch.int32, device=dev)
                valid = torch.tensor([0 if (failing == rank and j == ids[-1]) else 1], dtype=torch.int32, device=dev)
                store.append(_det(_global_batch(j, B, 7), dev), n_live=live, valid=valid)
            try:
                whole = gather_stores(store, plan, num_classes=3)
                out.append(("ok", [t.cpu().numpy() for t in whole.packed(3)], len(whole), whole.invalid_batches(), whole.row_capacity))
            except Exception as e:                                            # noqa: BLE001
                out.append((type(e).__name__, str(e)))
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:                                                    # noqa: BLE001
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()[-1500:]))


def _spawn(target, world, args, timeout=300):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = sorted((q.get(timeout=timeout) for _ in procs), key=lambda o: o[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank, res in out:
        assert not isinstance(res, str), (rank, res)
    return [res for _, res in out]


def _assert_gathered(res, n, B):
    want = _one_store_statement(n, B, 7)
    kind, got, scenes, invalid, row_capacity = res
    assert kind == "ok" and scenes == n and invalid == [] and row_capacity == max(want[0].shape[0], 1)
    for name, g, x in zip(("boxes", "scores", "labels", "off"), got, want):
        assert g.dtype == x.dtype and g.shape == x.shape and g.tobytes() == x.tobytes(), name


@pytest.fixture(scope="module")
def world2(cuda):
    """two processes, gloo, one GPU, no model: a good gather of 9 scenes, then one in which rank 1 leaves an invalid batch unrepaired"""
    return _spawn(_gather_worker, 2, ("gloo", [(9, 2, None), (9, 2, 1)]))


def test_world2_gather_equals_the_one_store_statement(world2):
    for rank in range(2):
        _assert_gathered(world2[rank][0], 9, 2)


def test_world2_a_failing_rank_raises_on_every_rank(world2):
    """... and hangs nobody: the workers came back within the time limit of the fixture, past the barrier behind the failed gather"""
    for rank in range(2):
        kind, text = world2[rank][1]
        assert kind == "RuntimeError" and "rank 1 of 2" in text and "still empty" in text, (rank, kind, text)


def test_world3_gather_with_an_empty_rank(cuda):
    res = _spawn(_gather_worker, 3, ("gloo", [(4, 2, None)]))                # two batches: rank 2 has none
    assert ShardPlan(4, 2, 3).scenes(2) == 0
    for rank in range(3):
        _assert_gathered(res[rank][0], 4, 2)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one GPU per rank: runs on a >= 2-GPU node only")
def test_world2_rccl_gather_equals_the_one_store_statement(cuda):
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = _spawn(_gather_worker, 2, ("nccl", [(9, 2, None), (9, 2, 1)]), timeout=600)
    for rank in range(2):
        _assert_gathered(res[rank][0], 9, 2)
        assert res[rank][1][0] == "RuntimeError" and "rank 1 of 2" in res[rank][1][1]


# ---- 6: end to end, two processes on one GPU ---------------------------------------------------------------------------------------
def _e2e_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import projects.mmdet3d_plugin  # noqa: F401
        from uni3detr_amd import datapath as dp
        from uni3detr_amd import evaluation as ev
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        w = _World(dev)                                                       # the same seeded model, captured from the same batches
        pts, gts, labs = w.small
        dpts, dgts, dlabs = w.dense
        batches = [pts[0:2], dpts, pts[4:5]]                                  # global batch 1 exceeds the captured level capacities ...
        gts, labs = gts[0:2] + dgts + gts[4:5], labs[0:2] + dlabs + labs[4:5]
        plan = ShardPlan(5, 2, world)
        ids = plan.batch_ids(rank)                                            # ... and lands on rank 1
        store = DetStore(plan.scenes(rank), w.max_num, 7, dev)
        before = w.step.fallbacks
        testing.test_dataset(w.step, (dp.pack_batch(batches[j]) for j in ids), store, reload=lambda j: batches[j],
                             on_batch=lambda j: torch.manual_seed(SEED + j), batch_ids=ids)
        repaired = w.step.fallbacks - before
        dist.init_process_group("gloo", rank=rank, world_size=world)
        whole = gather_stores(store, plan, num_classes=w.num_classes)
        e = ev.IndoorEvaluator(w.num_classes, device=dev)
        e.add_store(whole, gts, labs)
        out = dict(repaired=repaired, packed=[t.cpu().numpy() for t in whole.packed()], metrics=e.compute())
        if rank == 0:                                                         # the whole set alone, in this same process
            alone, metrics = _store_loop(w, batches, gts, labs, lambda i: batches[i])
            out.update(alone=[t.cpu().numpy() for t in alone.packed()], alone_metrics=metrics)
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:                                                    # noqa: BLE001
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()[-1500:]))


def test_sharded_dataset_loop_equals_the_one_process_loop(cuda):
    r0, r1 = _spawn(_e2e_worker, 2, (), timeout=600)
    assert r0["repaired"] == 0 and r1["repaired"] == 1                        # the repair happened on rank 1, before the gather
    want = r0["alone"]
    assert want[0].shape[0] > 0 and want[3].shape[0] == 6
    for name, res in (("rank 0", r0), ("rank 1", r1)):
        for field, g, x in zip(("boxes", "scores", "labels", "off"), res["packed"], want):
            assert g.dtype == x.dtype and g.shape == x.shape and g.tobytes() == x.tobytes(), (name, field)
        _same_dict(res["metrics"], r0["alone_metrics"])
