"""The acting paths of the QR-DQN head (csrc/kernels/qr_head.hip): the stand-alone acting launch
(``qr_infer_kernel`` with the fused actor step, what ``DeviceActor.step()`` / ``act_fused`` run) and
the acting blocks of the training launch (``qr_act_env_block``, one block per env).

* On synthetic quantile rows (the inputs of test_qr_head_gpu.py, qr_ref.py) with epsilon = 0, every env's
  appended action is the first argmax of the float64 quantile means of its row (dueling combined),
  for both launches; the transition lands at the cursor with the env's frame stack, the next frame
  slot and gamma; cursor, frame counter and ticket advance; with prioritized replay the E new
  leaves of the sum-tree hold the running max priority (the PER insert scratch of each kernel:
  behind Q in the inference kernel, the dynamic LDS of the acting blocks). Rows whose two best
  means lie within 1e-4 of the row's quantile range in the reference are left out, at most one in
  16 (asserted on the reference; row 8 is scaled by 30). The learner blocks of a training launch
  with acting blocks write bit for bit what the launch without them writes.
* On the network: the device actors' step inside the learner's launches writes the same
  transitions / frames / eps as the stand-alone acting launch with the same weights and RNG
  (test_executor_gpu.py::test_fused_acting_matches_separate_actor, for quantile nets; the noisy
  + prioritized case uses both kernels' PER scratch).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from head_ref import DEV, HID, dims as _dims, ext as _ext
from qr_ref import inputs as _inputs, quantiles64 as _quantiles64
from qr_ref import train as _qr_train

pytestmark = pytest.mark.gpu
CAP = 256


def _greedy64(rows, A, N, dueling):
    """(first argmax of the float64 quantile means [E], near-tie rows [E], means [E, A], largest |input| [E])."""
    th, mag = _quantiles64(rows, A, N, dueling)
    q = th.mean(-1)
    E = q.shape[0]
    best = np.zeros(E, dtype=np.int64)
    for e in range(E):
        for i in range(1, A):
            if q[e, i] > q[e, best[e]]:
                best[e] = i
    top = np.sort(q, axis=1)
    rng = th.reshape(E, -1).max(-1) - th.reshape(E, -1).min(-1)
    skip = (top[:, -1] - top[:, -2]) < 1e-4 * rng
    assert int(skip.sum()) * 16 <= E, ('near-ties in the reference: pick another seed', np.nonzero(skip)[0])
    return best, skip, q, mag


def _actor(A, E, per):
    """A fresh frame-mode replay and E greedy (epsilon = 0) device actors on it."""
    from dist_dqn_amd.actors.device_actor import DeviceActor
    from dist_dqn_amd.replay import DeviceReplay
    rep = DeviceReplay(CAP, (84, 84), 4, device=DEV, prioritized=per, seed=5)
    net = SimpleNamespace(arch=SimpleNamespace(num_actions=A), executor=None, noise=None)
    cfg = SimpleNamespace(init_random_action_prob=0.0, min_random_action_prob=0.0, random_action_explore_steps=1,
                          reward_discount=0.97)
    actor = DeviceActor(net, rep, cfg, num_envs=E, steps_per_call=1, seed=11, use_graph=False)
    ptrs, ints, f = actor._actor_args()
    return rep, actor, ptrs + ints, f


def _check_appended(rep, actor, E, best, skip, stacks0, f0, per):
    torch.cuda.synchronize()
    assert rep.cursor.tolist() == [E, f0 + 2 * E, E] and int(rep.size_dev) == E
    assert actor.env_frames == E and int(actor.ticket) == 0 and int(actor.rng[1]) == 1
    acts = rep.actions[:E].cpu().numpy()
    keep = ~skip
    assert (acts[keep] == best[keep]).all(), (np.nonzero(acts != best)[0], acts, best)
    assert (rep.actions[E:] == 0).all() and (rep.gammas[E:] == 1.0).all(), 'written beyond the E new transitions'
    assert torch.equal(rep.state_idx[:E], stacks0), 'the envs\' frame stacks'
    assert rep.next_idx[:E].tolist() == [f0 + 2 * e for e in range(E)]
    torch.testing.assert_close(rep.gammas[:E], torch.full((E,), 0.97, device=DEV), rtol=0, atol=0)
    assert set(rep.rewards[:E].tolist()) <= {-1.0, 0.0, 1.0}
    if per:
        t = rep.tree
        mp = float(t.max_p)
        leaves = t.sum[t.P:t.P + E + 1].cpu()
        assert mp > 0 and (leaves[:E] == mp).all() and float(leaves[E]) == 0.0, 'PER insert at the max priority'
        assert float(t.sum[1]) == pytest.approx(E * mp, rel=1e-6), 'sum-tree root'


# E, A, N, dueling, prioritized
ALONE = [(4, 6, 51, 1, 0), (4, 6, 51, 1, 1), (64, 18, 64, 1, 1), (9, 19, 33, 0, 1), (16, 4, 2, 1, 0), (1, 5, 32, 0, 1)]


@pytest.mark.parametrize('E,A,N,dueling,per', ALONE)
def test_qr_acting_launch_acts_on_the_quantile_means(E, A, N, dueling, per):
    rows = _inputs(E, A, N, dueling, False, 'none', 1.0, 7000 + 100 * A + N + E)['rows'][0]
    best, skip, qref, mag = _greedy64(rows, A, N, dueling)
    rep, actor, args, f = _actor(A, E, per)
    stacks0, f0 = actor.stacks.clone(), int(rep.cursor[1])
    r = rows.to(DEV).contiguous()
    q = torch.full((E * A + 8,), float('nan'), dtype=torch.float32, device=DEV)
    _ext('').qnet_qr_head([E, A, HID, int(dueling), 0, 1], [N], [1.0], [], [], [], [], [],
                          [0] * 7 + [q.data_ptr()] + [0] * 5, [], [], [], args, f, [r.data_ptr()], 0, [])
    _check_appended(rep, actor, E, best, skip, stacks0, f0, per)
    assert torch.isnan(q[E * A:]).all() and not torch.isnan(q[:E * A]).any()
    err = np.abs(q[:E * A].cpu().double().numpy().reshape(E, A) - qref)          # (test_qr_head_gpu.py's bound)
    assert (err <= ((3 * N + A + 4) if dueling else (N + 2)) * 2.0 ** -24 * mag[:, None]).all()


# E, A, N, dueling, double, prioritized (B = 24 learner rows)
FUSED = [(4, 6, 51, 1, 1, 0), (4, 6, 51, 1, 1, 1), (20, 18, 64, 1, 1, 1), (9, 19, 33, 0, 1, 1), (16, 4, 2, 0, 0, 0)]


@pytest.mark.parametrize('E,A,N,dueling,double,per', FUSED)
def test_qr_training_launch_acting_blocks_act_on_the_quantile_means(E, A, N, dueling, double, per):
    B = 24
    c = _inputs(B, A, N, dueling, double, 'rand', 1.0, 8000 + 100 * A + N + E)
    rows = _inputs(E, A, N, dueling, False, 'none', 1.0, 9000 + 100 * A + N + E)['rows'][0]
    best, skip, _, _ = _greedy64(rows, A, N, dueling)
    ext = _ext('')
    dout0, prio0, parts0 = _qr_train(ext, 'qnet_qr_head', c, torch.bfloat16)     # the same launch without acting blocks
    rep, actor, args, f = _actor(A, E, per)
    stacks0, f0 = actor.stacks.clone(), int(rep.cursor[1])
    _, _, KD = _dims(A, N, dueling)
    t = {k: c[k].to(DEV).contiguous() for k in ('rows', 'rew', 'done', 'gam', 'act', 'wts')}
    r = rows.to(DEV).contiguous()
    dout = torch.full(((B + 8) * KD,), -4096.0, dtype=torch.bfloat16, device=DEV)
    prio = torch.full((B + 8,), -4096.0, dtype=torch.float32, device=DEV)
    parts = torch.full((72,), -4096.0, dtype=torch.float32, device=DEV)
    io = [t['act'].data_ptr(), t['rew'].data_ptr(), t['done'].data_ptr(), t['gam'].data_ptr(), t['wts'].data_ptr(), 0,
          prio.data_ptr()] + [0] * 6
    lg = [t['rows'][i].data_ptr() for i in range(3 if double else 2)] + [r.data_ptr()]
    act_h = torch.zeros(E * 2 * HID, dtype=torch.bfloat16, device=DEV)   # (the QR head reads the rows, not h)
    ext.qnet_qr_head([B, A, HID, int(dueling), 0, 0], [N], [1.0], [], [], [], [], [], io, [], [], [], args, f, lg,
                     act_h.data_ptr(), [parts.data_ptr(), dout.data_ptr()])
    _check_appended(rep, actor, E, best, skip, stacks0, f0, per)
    assert torch.equal(prio.cpu(), prio0) and torch.equal(parts.cpu(), parts0), 'learner blocks beside acting blocks'
    assert torch.equal(dout.cpu().view(torch.uint8), dout0.view(torch.uint8))


def test_qr_head_refuses_more_than_32_actions():
    """One template instance holds at most 32 action rows: refused before any launch."""
    r = torch.zeros(4, _dims(33, 8, 0)[2], device=DEV)
    q = torch.full((4 * 33,), float('nan'), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match='1..32 actions'):
        _ext('').qnet_qr_head([4, 33, HID, 0, 0, 1], [8], [1.0], [], [], [], [], [],
                              [0] * 7 + [q.data_ptr()] + [0] * 5, [], [], [], [], [], [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    assert torch.isnan(q).all()


QRD = '--quantile --dueling'


@pytest.mark.parametrize('extra', [QRD, QRD + ' --init_random_action_prob=0 --min_random_action_prob=0',
                                   QRD + ' --double_dqn --noisy --prioritized_replay'])
def test_qr_fused_acting_matches_separate_actor(extra):
    """The device actors' step inside the learner launches writes the same transitions / frames /
    eps as the stand-alone act_fused path with the same weights and RNG (the second case: every
    action greedy on the same first frames, so the two kernels' Q rows decide all twelve)."""
    from dist_dqn_amd.actors.device_actor import DeviceActor
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    outs = []
    for fused in (False, True):
        cfg = preset('nature', 'Pong-v0', '--seed=4 --backend=hip --dtype=bf16 --replay_memory_capacity=65536 ' + extra)
        net = Network.create_network(cfg, (84, 84, 4), 6, device=DEV)
        assert net.executor.quantile
        greedy = '--init_random_action_prob=0' in extra
        if greedy:                             # weights under which the actions' Q values lie well apart
            g = torch.Generator(device=DEV).manual_seed(7)
            net.online.flat.normal_(0.0, 0.03, generator=g)
            net.target.flat.normal_(0.0, 0.03, generator=g)
            net.refresh_packed()
        rep = DeviceReplay(65536, (84, 84), 4, device=DEV, seed=5, prioritized=cfg.prioritized_replay)
        rep.fill_synthetic(65536, 6, seed=5)
        torch.manual_seed(123)                 # the envs' first frames (DeviceActor draws them from torch's RNG)
        actor = DeviceActor(net, rep, cfg, num_envs=4, steps_per_call=1, seed=11, use_graph=False)
        assert actor.can_fuse(cfg.minibatch_size)
        ln = Learner(net, rep, cfg, use_graph=False, actor=actor if fused else None)
        assert (ln.actor is not None) == fused
        for _ in range(3):
            if not fused:
                actor.step()
            ln.step()
        torch.cuda.synchronize()
        cur = rep.cursor.clone()
        t0 = int(cur[0]) - 12
        outs.append(dict(cursor=cur, actions=rep.actions[t0:t0 + 12].clone(), rewards=rep.rewards[t0:t0 + 12].clone(),
                         eps=actor.eps.clone(), frames_done=actor.frames_done.clone(), stacks=actor.stacks.clone(),
                         frame=rep.frames[int(actor.stacks[0, -1])].clone()))
    a, b = outs
    for k in a:
        assert torch.equal(a[k], b[k]), k
