"""The detection store without a GPU: the header / export / binding triple of u3d_det_store_append and u3d_det_store_pack, their argument
checks (answered before any launch, so they run here), the NumPy restatement of tests/det_store_ref.py against plain concatenation of
per-scene lists (padding scenes, invalid calls, a refused call, a repair, a pack after a repair), and the loop of
uni3detr_amd.testing.test_dataset on stub step / store objects."""
import ctypes as C

import numpy as np
import pytest

import det_store_ref as ref
from test_abi_cpu import _Host
from uni3detr_amd import abi
from uni3detr_amd import native as nv
from uni3detr_amd import testing

P, I = C.c_void_p, C.c_int32
OK, ARG, UNSUPPORTED = 0, -1, -2


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    protos = abi.load().prototypes
    assert protos["u3d_det_store_append"] == (I, [P] * 4 + [I] * 3 + [P] * 9 + [I] * 3 + [P])
    assert protos["u3d_det_store_pack"] == (I, [P] * 4 + [I] * 4 + [P] * 3 + [I, P, P, P])
    raw = C.CDLL(nv.LIB_PATH)
    for name in ("u3d_det_store_append", "u3d_det_store_pack"):
        assert name in nv.exported_symbols() and hasattr(raw, name)
        fn = getattr(nv.lib(), name)
        assert fn.restype is protos[name][0] and list(fn.argtypes) == protos[name][1]
    assert callable(nv.det_store_append) and callable(nv.det_store_pack)


def test_append_return_codes():
    h = _Host(16)

    def call(batch=2, K=5, D=7, R=64, S=8, M=4, null=None, invalid=True):
        a = [None if null == k else h[k] for k in range(4)]                 # boxes scores labels count
        st = [None if null == 4 + k else h[4 + k] for k in range(5)]        # store boxes scores labels table cursor
        return nv.lib().u3d_det_store_append(*a, batch, K, D, None, None, None, *st, h[9] if invalid else None, R, S, M, None)

    assert call(D=8) == ARG and call(batch=0) == ARG and call(K=0) == ARG and call(R=0) == ARG and call(S=0) == ARG and call(M=-1) == ARG
    for k in range(9):
        assert call(null=k) == ARG, k
    assert call(invalid=False) == ARG                                       # M > 0 needs the list
    assert call(batch=65536) == UNSUPPORTED and call(K=nv.DET_TAIL_MAX_K + 1) == UNSUPPORTED
    assert call(R=(2 ** 31) // 7 + 1) == UNSUPPORTED and call(D=9, R=(2 ** 31) // 9 + 1) == UNSUPPORTED
    assert call(D=8, batch=65536) == ARG                                    # argument checks come before shape checks


def test_pack_return_codes():
    h = _Host(16)

    def call(n=3, R=64, D=7, rows=10, null=None):
        a = [None if null == k else h[k] for k in range(4)]                 # store boxes scores labels table
        o = [None if null == 4 + k else h[4 + k] for k in range(5)]         # out boxes scores labels | off bad
        return nv.lib().u3d_det_store_pack(*a, n, R, D, 0, o[0], o[1], o[2], rows, o[3], o[4], None)

    assert call(D=8) == ARG and call(n=-1) == ARG and call(R=0) == ARG and call(rows=-1) == ARG
    for k in range(9):
        assert call(null=k) == ARG, k
    assert call(R=(2 ** 31) // 7 + 1) == UNSUPPORTED and call(rows=(2 ** 31) // 7 + 1) == UNSUPPORTED


def test_store_is_gpu_only():
    from uni3detr_amd.det_store import DetStore
    with pytest.raises(RuntimeError, match="GPU"):
        DetStore(4, 5, 7, "cpu")


# ---- the restatement against plain concatenation --------------------------------------------------------------------------------------
def _scene_list(det, n):
    b, s, l, c = det
    return [(b[i, :c[i]], s[i, :c[i]], l[i, :c[i]]) for i in range(n)]


def _same_pack(store, want_scenes, D):
    got = store.pack()
    want = ref.concat_lists(want_scenes, D)
    for name, g, w in zip(("boxes", "scores", "labels", "off"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    assert got[4].tolist() == [0, 0]


@pytest.mark.parametrize("D", [7, 9])
def test_restatement_appends_in_scene_order_and_skips_padding(D):
    rng = np.random.default_rng(D)
    st = ref.RefStore(12, 12 * 5, D, 4)
    want = []
    for n_live in (3, 1, 0, 2, None):
        det = ref.random_det(rng, 3, 5, D)
        assert st.append(*det, n_live=n_live)
        want += _scene_list(det, 3 if n_live is None else n_live)
    assert st.cursor.tolist() == [9, sum(w[1].shape[0] for w in want), 0, 0]
    assert np.array_equal(st.table[:9, 0], ref.concat_lists(want, D)[3][:-1]) and (st.table[9:] == -1).all()
    assert np.isnan(st.boxes[st.cursor[1]:]).all() and (st.labels[st.cursor[1]:] == -1).all()        # nothing past the used rows
    _same_pack(st, want, D)


def test_restatement_reads_counts_clamped():
    rng = np.random.default_rng(1)
    st = ref.RefStore(4, 20, 7, 2)
    b, s, l, _ = ref.random_det(rng, 3, 5, 7, counts=[5, 5, 5])
    assert st.append(b, s, l, np.array([-2, 9, 3], np.int32))
    assert st.table[:3].tolist() == [[0, 0], [0, 5], [5, 3]] and st.cursor.tolist() == [3, 8, 0, 0]


def test_restatement_invalid_calls_record_empty_scenes():
    rng = np.random.default_rng(2)
    st = ref.RefStore(12, 60, 7, 2)
    a, b, c, d, e = (ref.random_det(rng, 3, 5, 7) for _ in range(5))
    st.append(*a)
    st.append(*b, n_live=2, valid=0)
    st.append(*c, valid=1)
    st.append(*d, n_live=0, valid=0)               # nothing to record: not counted
    st.append(*e, n_live=1, valid=0)
    st.append(*e, n_live=1, valid=0)               # a third invalid call: counted, no longer listed
    empty = (np.zeros((0, 7), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
    assert st.cursor.tolist() == [10, int(a[3].sum() + c[3].sum()), 3, 0]
    assert st.invalid.tolist() == [[3, 2], [8, 1]]
    _same_pack(st, _scene_list(a, 3) + [empty] * 2 + _scene_list(c, 3) + [empty] * 2, 7)


def test_restatement_refuses_whole_calls():
    rng = np.random.default_rng(3)
    st = ref.RefStore(4, 20, 7, 2)
    a = ref.random_det(rng, 3, 5, 7)
    assert st.append(*a)
    before = {k: v.copy() for k, v in st.arrays().items()}
    assert not st.append(*ref.random_det(rng, 3, 5, 7))                    # 6 scenes into 4
    after = st.arrays()
    assert after["cursor"].tolist() == before["cursor"][:3].tolist() + [1]
    for k in ("boxes", "scores", "labels", "table", "invalid"):
        assert np.array_equal(after[k], before[k], equal_nan=True), k
    st = ref.RefStore(8, 7, 7, 2)                                           # rows: 5 + 0 + 3 do not go into 7
    assert not st.append(*ref.random_det(rng, 3, 5, 7, counts=[5, 0, 3])) and st.cursor.tolist() == [0, 0, 0, 1]
    assert st.append(*ref.random_det(rng, 3, 5, 7, counts=[5, 0, 2])) and st.cursor.tolist() == [3, 7, 0, 1]


def test_restatement_repair_and_pack_after_it():
    rng = np.random.default_rng(4)
    a, b, c = (ref.random_det(rng, 3, 5, 7) for _ in range(3))
    st = ref.RefStore(9, 60, 7, 2)
    st.append(*a)
    st.append(*b, valid=0)
    st.append(*c)
    assert st.invalid[0].tolist() == [3, 3]
    assert st.append(*b, scene_ids=np.array([3, 4, 5], np.int32))
    assert st.cursor.tolist() == [9, int(a[3].sum() + b[3].sum() + c[3].sum()), 1, 0]
    _same_pack(st, _scene_list(a, 3) + _scene_list(b, 3) + _scene_list(c, 3), 7)            # = the all-valid sequence
    # a second repair of scene 4 leaves its first rows unreferenced: they do not appear in the pack
    d = ref.random_det(rng, 3, 5, 7, counts=[2, 5, 0])
    used = int(st.cursor[1])
    assert st.append(*d, n_live=1, scene_ids=np.array([4, 0, 0], np.int32)) and st.cursor[1] == used + 2
    want = _scene_list(a, 3) + _scene_list(b, 3) + _scene_list(c, 3)
    want[4] = _scene_list(d, 1)[0]
    _same_pack(st, want, 7)
    # a scene id past the cursor, and an invalid repair, are refused whole
    assert not st.append(*d, scene_ids=np.array([0, 9, 1], np.int32)) and not st.append(*d, valid=0, scene_ids=np.array([0, 1, 2], np.int32))
    assert st.cursor.tolist() == [9, used + 2, 1, 2]
    _same_pack(st, want, 7)


def test_restatement_pack_flags():
    rng = np.random.default_rng(5)
    st = ref.RefStore(3, 15, 7, 1)
    b, s, l, c = ref.random_det(rng, 3, 5, 7, counts=[2, 0, 3])
    l[2, 1] = 7
    s[0, 1] = np.inf
    st.append(b, s, l, c)
    assert st.pack(num_classes=0)[4].tolist() == [1, 0] and st.pack(num_classes=8)[4].tolist() == [1, 0]
    assert st.pack(num_classes=7)[4].tolist() == [1, 1] and st.pack(n_scenes=2, num_classes=7)[4].tolist() == [1, 0]


# ---- the loop on stubs ------------------------------------------------------------------------------------------------------------
class _Scalar:
    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


class _Inf:
    def __init__(self, log):
        self.log = log

    def simple_test_batched(self, img_metas, points, on_device=False):
        assert img_metas is None and on_device is True
        self.log.append(("eager", list(points)))
        return ("eager-det", list(points))


class _Step:
    batch_size = 2

    def __init__(self, log):
        self.log, self.inf, self.fallbacks = log, _Inf(log), 0
        self.det = self.valid = self.n_live = None

    def run(self, batch):
        self.log.append(("run", batch))
        self.det, self.valid, self.n_live = ("det", len(self.log)), "valid", "n_live"
        return self.det


class _Store:
    def __init__(self, log, invalid=(), held=0):
        self.log, self._invalid, self.held = log, list(invalid), held

    def __len__(self):
        return self.held

    def append(self, det, n_live=None, valid=None):
        self.log.append(("append", det, n_live, valid))

    def invalid_batches(self):
        self.log.append(("invalid_batches",))
        return list(self._invalid)

    def put(self, first, dets):
        self.log.append(("put", first, dets))


def _dict_batch(n, tag):
    return dict(points=tag, scene_off=_Scalar(n + 1))


def test_loop_order_and_partial_last_batch(monkeypatch):
    log = []
    step, store = _Step(log), _Store(log)
    monkeypatch.setattr(testing, "_scenes", lambda b: [b["points"] + "0"] if isinstance(b, dict) else list(b))
    full = [_dict_batch(2, "a"), _dict_batch(2, "b")]
    out = testing.test_dataset(step, iter(full + [_dict_batch(1, "c")]), store, on_batch=lambda i: log.append(("on_batch", i)))
    assert out is store and step.fallbacks == 0
    kinds = [e[0] for e in log]
    assert kinds == ["on_batch", "run", "append"] * 3 + ["invalid_batches"]
    assert [e[1] for e in log if e[0] == "on_batch"] == [0, 1, 2]
    runs = [e[1] for e in log if e[0] == "run"]
    assert runs[0] is full[0] and runs[1] is full[1]                       # packed dicts go through as they are
    assert runs[2] == ["c0"]                                               # the partial one as a list: run() pads and gates it
    for e, r in zip([e for e in log if e[0] == "append"], (2, 5, 8)):
        assert e[1:] == (("det", r), "n_live", "valid")                    # the step's own outputs of THAT run
    # lists work as batches too, and no on_batch is fine
    log.clear()
    testing.test_dataset(step, [["p", "q"], ["r"]], store)
    assert [e[0] for e in log] == ["run", "append"] * 2 + ["invalid_batches"]


def test_loop_repairs_invalid_batches():
    log = []
    step, store = _Step(log), _Store(log, invalid=[(2, 2), (4, 1)])
    reloaded = {1: ["r1a", "r1b"], 2: ["r2"]}

    def reload(i):
        log.append(("reload", i))
        return reloaded[i]

    testing.test_dataset(step, [["a", "b"], ["c", "d"], ["e"]], store, reload=reload, on_batch=lambda i: log.append(("on_batch", i)))
    tail = log[log.index(("invalid_batches",)) + 1:]
    assert tail == [("reload", 1), ("on_batch", 1), ("eager", ["r1a", "r1b"]), ("put", 2, ("eager-det", ["r1a", "r1b"])),
                    ("reload", 2), ("on_batch", 2), ("eager", ["r2"]), ("put", 4, ("eager-det", ["r2"]))]
    assert step.fallbacks == 2
    # a store that already held 10 scenes: this loop's batches start there, an earlier range is not this loop's to repair
    log.clear()
    step, store = _Step(log), _Store(log, invalid=[(4, 2), (12, 2)], held=10)
    testing.test_dataset(step, [["a", "b"], ["c", "d"]], store, reload=lambda i: reloaded[i])
    assert [e for e in log if e[0] == "put"] == [("put", 12, ("eager-det", ["r1a", "r1b"]))] and step.fallbacks == 1


def test_loop_raises_without_reload_and_on_a_wrong_reload():
    log = []
    with pytest.raises(RuntimeError, match="batch 1 .*no reload"):
        testing.test_dataset(_Step(log), [["a", "b"], ["c", "d"]], _Store(log, invalid=[(2, 2)]))
    with pytest.raises(RuntimeError, match="returned 1 scenes"):
        testing.test_dataset(_Step(log), [["a", "b"], ["c", "d"]], _Store(log, invalid=[(2, 2)]), reload=lambda i: ["x"])
    with pytest.raises(RuntimeError, match="did not append"):
        testing.test_dataset(_Step(log), [["a", "b"], ["c", "d"]], _Store(log, invalid=[(1, 2)]), reload=lambda i: ["x", "y"])
    assert not [e for e in log if e[0] == "put"]
