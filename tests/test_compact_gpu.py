"""u3d_compact_rows / native.compact_rows against a NumPy boolean-mask compaction, bit for bit: the two row sizes the evaluators use
(16 x f32 = 64 B, 12 x f64 = 96 B), no rows, one row kept or dropped, and 300 rows - 4800 / 7200 words, several 256-thread workgroups with
a partial last one - under every / no / every other flag, over scenes of which the first, a middle and the last are empty."""
import numpy as np
import pytest
import torch

from uni3detr_amd import native as nv
from uni3detr_amd.eval_common import offsets

pytestmark = pytest.mark.gpu
ROWS = {64: (torch.float32, 16), 96: (torch.float64, 12)}
CASES = [("none", [], []), ("one kept", [1], [1]), ("one dropped", [1], [0]),
         ("all", [0, 120, 0, 180, 0], None), ("no flag", [0, 120, 0, 180, 0], None), ("alternating", [0, 120, 0, 180, 0], None)]


def _flags(name, n):
    return {"all": np.ones(n, np.int32), "no flag": np.zeros(n, np.int32), "alternating": (np.arange(n) % 2).astype(np.int32)}[name]


@pytest.mark.parametrize("row_bytes", sorted(ROWS))
@pytest.mark.parametrize("name,counts,flags", CASES, ids=[c[0] for c in CASES])
def test_compact_rows_equals_a_boolean_mask(cuda, row_bytes, name, counts, flags):
    dtype, cols = ROWS[row_bytes]
    n = sum(counts)
    valid = np.asarray(flags, np.int32) if flags is not None else _flags(name, n)
    words = np.random.default_rng(row_bytes + n).integers(-2 ** 31, 2 ** 31, size=(n, row_bytes // 4), dtype=np.int64).astype(np.int32)
    as_np = np.float32 if dtype == torch.float32 else np.float64
    rec = torch.from_numpy(words.view(as_np)).to(cuda)                      # every bit pattern, NaNs included: rows are moved, not read
    assert rec.shape == (n, cols) and rec.element_size() * cols == row_bytes
    off = offsets(counts)
    dvalid = torch.from_numpy(valid).to(cuda)
    out, new_off = nv.compact_rows(rec, dvalid, torch.from_numpy(off).to(cuda))
    want = torch.from_numpy(words[valid.astype(bool)]).to(cuda)
    assert out.dtype == dtype and out.shape == (int(valid.sum()), cols) and torch.equal(out.view(torch.int32), want)
    kept = [int(valid[a:b].sum()) for a, b in zip(off[:-1], off[1:])]
    assert new_off.dtype == torch.int32 and torch.equal(new_off, offsets(kept, cuda))
    # the entry itself, into a buffer of n + 1 rows of a sentinel: the kept rows in front, nothing written behind them
    m = int(valid.sum())
    pos = torch.from_numpy((np.cumsum(valid) - valid).astype(np.int32)).to(cuda)
    raw = torch.full((n + 1, row_bytes // 4), -7, dtype=torch.int32, device=cuda)
    rc = nv.lib().u3d_compact_rows(nv._ptr(rec) if n else None, nv._ptr(dvalid) if n else None,
                                   nv._ptr(pos) if n else None, n, row_bytes, nv._ptr(raw), nv._stream())
    assert rc == 0 and torch.equal(raw[:m], want) and bool((raw[m:] == -7).all())


@pytest.mark.parametrize("row_bytes", [0, 6, -4])
def test_a_row_size_that_is_no_positive_multiple_of_4_is_refused(cuda, row_bytes):
    rec = torch.arange(8, dtype=torch.int32, device=cuda).reshape(2, 4)
    valid = torch.ones(2, dtype=torch.int32, device=cuda)
    pos = torch.arange(2, dtype=torch.int32, device=cuda)
    out = torch.full((2, 4), -7, dtype=torch.int32, device=cuda)
    call = lambda n, rb: nv.lib().u3d_compact_rows(nv._ptr(rec), nv._ptr(valid), nv._ptr(pos), n, rb, nv._ptr(out), nv._stream())    # noqa: E731
    assert call(2, row_bytes) == -1 and call(0, row_bytes) == -1 and call(-1, 16) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                          # nothing was launched
    assert call(2, 16) == 0 and torch.equal(out, rec)
