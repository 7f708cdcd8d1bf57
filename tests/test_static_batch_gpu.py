"""GPU: static_batch.validity_flag alone - the one device flag TrainStep and InferenceStep gate a replay on.  The model is a
SimpleNamespace carrying what the function reads."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from uni3detr_amd import static_batch as sb

pytestmark = pytest.mark.gpu


def test_validity_flag_is_set_exactly_when_a_source_is(cuda):
    def i32(*v):
        return torch.tensor(v, dtype=torch.int32, device=cuda)

    caps = [256, 256]
    for over, timed_out, cut in itertools.product((False, True), repeat=3):
        # last_level_counts[0] is the voxel list, which the strided levels' capacities do not cover
        enc = SimpleNamespace(last_level_counts=[i32(10 ** 6), i32(256), i32(257 if over else 256)])
        model = SimpleNamespace(pts_middle_encoder=enc, pts_voxel_encoder=None)
        out = torch.full((1,), 7.0, device=cuda)                       # stale: every call overwrites it
        sb.validity_flag(model, caps, i32(3 if timed_out else 0, 9), torch.tensor([float(cut)], device=cuda), out)
        assert (out.item() > 0) == (over or timed_out or cut), (over, timed_out, cut, out.item())
    # nothing to test: zeroed, then the ingest flag alone
    model = SimpleNamespace(pts_middle_encoder=SimpleNamespace(last_level_counts=[]), pts_voxel_encoder=None)
    for cut in (0.0, 1.0):
        out = torch.full((1,), 7.0, device=cuda)
        sb.validity_flag(model, None, None, torch.tensor([cut], device=cuda), out)
        assert out.item() == cut
    out = torch.full((1,), 7.0, device=cuda)
    sb.validity_flag(model, None, None, None, out)
    assert out.item() == 0.0
