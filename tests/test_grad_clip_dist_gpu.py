"""A clipped data-parallel run, rehearsed with two ranks on one GPU (gloo control plane, the xgmi
peer-to-peer kernels for the data, as tests/test_dist_gpu.py runs its ranks): 10 clipped steps of the
Nature net, after which the replicas and the reported norms are bit-equal and the error words clean.

The clip sits after the all-reduce, on a buffer that holds the same bits on every rank (the fc weight
gradient from the all-gathered rows in one fixed-order launch, the rest all-reduced), and its
summation order depends on the buffer's size alone: so do the norm, the scale and the update."""
import os
import socket
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT_S = 90.0


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, errq):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK='0', DQN_DIST_BACKEND='gloo')
        import faulthandler
        import sys
        faulthandler.dump_traceback_later(CHILD_TIMEOUT_S - 10.0, exit=False)
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from dist_dqn_amd.config import preset
        from dist_dqn_amd.learner import Learner
        from dist_dqn_amd.models.network import Network
        from dist_dqn_amd.parallel import broadcast_state, check_state_equal, init_distributed
        from dist_dqn_amd.replay import DeviceReplay
        # (a bound below this freshly initialised net's gradient norm, ~1e-4: the steps are clipped)
        cfg = preset('nature', 'Pong-v0', '--dtype=bf16 --seed=%d --backend=hip --replay_memory_capacity=2048 '
                     '--allreduce=xgmi --max_grad_norm=1e-5' % (3 + rank))
        ctx = init_distributed(cfg, device='cuda')
        assert ctx.world_size == world and ctx.backend == 'gloo' and ctx.device.index == 0
        net = Network.create_network(cfg, (84, 84, 4), 6, num_replicas=world, device=ctx.device)
        broadcast_state(ctx, net)
        rep = DeviceReplay(2048, (84, 84), 4, device=ctx.device, seed=rank)
        rep.fill_synthetic(2048, 6, seed=rank)          # different data per rank
        ln = Learner(net, rep, cfg, ctx)
        assert ln.use_graph and ln.reducer.mode == 'xgmi'
        # the low-rank fc exchange stays on; nothing is left to the optimizer launch
        assert ln._lowrank is not None
        assert not ln._defer_fc and not ln._defer_wgrad and not ln._dp_fused and not ln._det_wgrad
        clipped = 0
        for step in range(10):                          # 2 eager warm-up steps, then graphs
            ln.step()
            torch.cuda.synchronize()
            st = net._clip_stats.cpu()
            assert float(st[0]) > 0.0 and 0.0 < float(st[1]) <= 1.0, (step, st)
            assert (float(st[1]) < 1.0) == (float(st[0]) > float(torch.tensor(1e-5))), (step, st)
            clipped += float(st[1]) < 1.0
            norms = [torch.zeros(1) for _ in range(world)]
            dist.all_gather(norms, ln.grad_norm.view(1).cpu())
            assert all(torch.equal(norms[0].view(torch.int32), t.view(torch.int32)) for t in norms), (step, norms)
        assert clipped >= 5, 'most steps of this run are clipped (eager and graph steps): %d' % clipped
        assert len(ln._graphs) == 1, 'the xgmi DP step is one graph'
        assert torch.isfinite(ln.loss).all() and int(net.global_step) == 10
        ln.reducer.check()                              # a timed-out peer wait raises here
        ln._device_checks()
        eq = check_state_equal(ctx, net)
        assert all(eq.values()), 'replicas diverged: %s' % eq
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001 - report to the parent
        import traceback
        errq.put('rank %d: %s\n%s' % (rank, e, traceback.format_exc()))
        raise


def test_two_ranks_one_gpu_clipped_replicas_and_norms_bit_equal():
    ctx = mp.get_context('spawn')
    errq = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, errq)) for r in range(2)]
    started = []
    for p in procs:
        p.start()
        started.append(time.monotonic())
    for p, t0 in zip(procs, started):                   # each child under its own time limit
        p.join(timeout=max(0.0, t0 + CHILD_TIMEOUT_S - time.monotonic()))
    alive = [p for p in procs if p.is_alive()]
    for p in alive:
        p.kill()
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not alive, 'rank(s) hung'
    assert not errs, '\n'.join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
