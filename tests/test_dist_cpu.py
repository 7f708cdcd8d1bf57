"""CPU, world size 2, gloo: the N>1 specific host logic - the fused scalar all-reduces of the loss / log-vars, and the reductions of
uni3detr_amd.trainer.TrainStep as bench.py runs them for N > 1 (flat gradient buffer averaged in THREE buckets in reverse layer
order - neck + head, SECOND3D, sparse encoder - the first two asynchronously, each in flight under the backward phase that follows it
(the two-bucket plan of rounds 3-5 is still covered); ONE small message per step carrying the positive counts and the capacity flag),
called as unbound methods on a CPU stand-in that holds the attributes they touch."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import projects.mmdet3d_plugin  # noqa: F401
        from uni3detr_amd.plugin.detector import Uni3DETR
        from uni3detr_amd.plugin.head import reduce_mean_
        # (1) per-layer positive counts: one vector all-reduce == mmdet reduce_mean applied per layer
        npos = torch.tensor([48.0, 40.0, 8.0]) * (rank + 1)
        got = reduce_mean_(npos.clone())
        assert torch.allclose(got, torch.tensor([48.0, 40.0, 8.0]) * 1.5)
        # (2) _parse_losses: loss = sum of 'loss' keys (local), log vars = rank means, one message
        det = Uni3DETR.__new__(Uni3DETR)
        losses = {"loss_cls": torch.tensor(1.0 + rank), "loss_bbox": torch.tensor(2.0), "d0.loss_cls": torch.tensor(3.0 * (rank + 1)),
                  "acc": torch.tensor(10.0 * rank)}
        loss, logs = Uni3DETR._parse_losses(det, losses)
        assert abs(float(loss) - (1.0 + rank + 2.0 + 3.0 * (rank + 1))) < 1e-6            # local loss drives backward
        assert abs(float(logs["loss_cls"]) - 1.5) < 1e-6 and abs(float(logs["acc"]) - 5.0) < 1e-6
        assert abs(float(logs["loss"]) - (1.5 + 2.0 + 4.5)) < 1e-6
        # (3) TrainStep's own reductions (bench.py, N > 1): the flat gradient is averaged in two buckets - [enc_end:) asynchronously,
        #     then [:enc_end) - and equals the mean of the ranks' local gradients element for element; the per-step message
        #     averages the positive counts and turns ANY rank's capacity flag into a positive flag on every rank
        from types import SimpleNamespace
        from uni3detr_amd.trainer import TrainStep
        g = torch.Generator().manual_seed(7)
        local = [torch.randn(1000, generator=g) * (r + 1) for r in range(world)]
        class _Stub(SimpleNamespace):                      # the reductions call each other through self
            _comm_view = TrainStep._comm_view
            _all_reduce_slice = TrainStep._all_reduce_slice
            _launch_bucket = TrainStep._launch_bucket
        st = _Stub(dist_on=True, world=world, flat_grad=local[rank].clone(), enc_end=384, bb_end=384, three_phase=False, grad_comm_dtype=torch.float32,
                   _comm=None, comm_diag=False, _msg=torch.tensor([30.0, 20.0, 10.0, 1.0 if rank == 1 else 0.0]) * torch.tensor([rank + 1.0] * 3 + [1.0]))
        st._works = []
        TrainStep._reduce_grads_a(st)
        assert len(st._works) == 1 and st._works[0][2:] == (384, 1000)
        TrainStep._reduce_grads_b(st)
        assert not st._works and torch.allclose(st.flat_grad, sum(local) / world, atol=1e-6)
        # (3a) the three-bucket plan (round 6): [bb_end:) after the head / FPN backward, [enc_end:bb_end) after SECOND3D's, [:enc_end) last;
        #      two reductions in flight at once; element for element the mean of the local gradients, identical to the single-bucket result
        s3 = _Stub(dist_on=True, world=world, flat_grad=local[rank].clone(), enc_end=100, bb_end=640, three_phase=True, grad_comm_dtype=torch.float32,
                   _comm=None, comm_diag=False)
        s3._works = []
        TrainStep._reduce_grads_a(s3)
        TrainStep._reduce_grads_m(s3)
        assert [w[2:] for w in s3._works] == [(640, 1000), (100, 640)]
        TrainStep._reduce_grads_b(s3)
        assert not s3._works and torch.equal(s3.flat_grad, st.flat_grad)
        st2 = _Stub(dist_on=True, world=world, flat_grad=local[rank].clone(), grad_comm_dtype=torch.float32, _comm=None)
        TrainStep._reduce_grads(st2)
        assert torch.allclose(st2.flat_grad, st.flat_grad, atol=1e-6)
        # (3b) the bf16 exchange option: same buckets, staged through a bf16 buffer - the mean to bf16 precision, identical on all ranks
        st3 = _Stub(dist_on=True, world=world, flat_grad=local[rank].clone(), enc_end=384, bb_end=700, three_phase=True, _comm=None, comm_diag=False)
        st3.grad_comm_dtype = torch.bfloat16
        st3._works = []
        TrainStep._reduce_grads_a(st3)
        TrainStep._reduce_grads_m(st3)
        TrainStep._reduce_grads_b(st3)
        exact = sum(local) / world
        assert not st3._works and float((st3.flat_grad - exact).abs().max()) <= 2.0 ** -7 * float(exact.abs().max())
        gathered = [torch.empty_like(st3.flat_grad) for _ in range(world)]
        dist.all_gather(gathered, st3.flat_grad)
        assert all(torch.equal(gathered[0], t) for t in gathered)
        TrainStep._reduce_num_pos(st)
        assert torch.allclose(st._msg[:3], torch.tensor([45.0, 30.0, 15.0])) and float(st._msg[3]) > 0.0      # rank 1's overflow holds rank 0 too
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_world2_gloo_scalar_reductions_and_trainstep_buckets():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(60)
    assert sorted(res) == [(0, "ok"), (1, "ok")], res
