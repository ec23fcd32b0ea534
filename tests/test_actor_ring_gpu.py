"""The device actor step and the replay rings it writes against the exact host model
(tests/actor_ref.py): after EVERY step every state tensor -- tables, stacks, cursors, eps, rng, the
env-frame counter, the ticket and the whole frame ring -- equals the model with ``torch.equal``.
No tolerance anywhere in this file: the path is integer Philox plus fp32 subtractions and compares.

The stand-alone kernel is driven directly (``ext.actor_step`` with crafted Q rows, no network) at
small shapes: 4 x 4 and 4 x 8 frames (H W stays a multiple of 16: ``write_random_frame`` stores
16-byte words), C = 23 / 24 (C = 93 / 94 where E = 70, as the kernel needs E <= C), K = 1 .. 4,
A in {2, 6, 18}, E in {1, 3, 8, 70} (70: more than 64 blocks through the arrival ticket), p_done =
0.3, enough steps to wrap the transition ring three times and the frame ring once. Then: the gather
and stack kernels for K = 1 .. 4, the sum-tree insertion of the new transitions, the integrity of
the frame ring through ``DeviceReplay`` / ``DeviceActor`` (the ring ``reserve_writers`` allocates),
and the fused acting path of the head kernel on the Nature net.
"""
import numpy as np
import pytest
import torch

import actor_ref as AR
import philox_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GAMMA = 0.99
TABLES = ('state_idx', 'next_idx', 'actions', 'rewards', 'dones', 'gammas')
STATE = ('stacks', 'cursor', 'size_dev', 'eps', 'rng', 'frames_done')


def _ext():
    from dist_dqn_amd.ops import _ext
    return _ext.load(required=True)


def _upload(m, hw):
    """The model's state as device tensors (frames [F, H, W]) + a zero ticket."""
    st = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in m.tensors().items()}
    st['frames'] = st['frames'].view(m.F, hw[0], hw[1])
    st['ticket'] = torch.zeros(1, dtype=torch.int32, device=DEV)
    return st


def _actor_step(ext, st, q, p_done, tree=None):
    args = [torch.from_numpy(q).to(DEV), st['frames'], st['stacks'], st['cursor'], st['size_dev'], st['state_idx'],
            st['next_idx'], st['actions'], st['rewards'], st['dones'], st['gammas'], st['eps'], st['rng'],
            st['ticket'], st['frames_done'], GAMMA, float(p_done)]
    if tree is not None:
        ext.actor_step(*args, tree=[tree.sum, tree.min, tree.max_p])
    else:
        ext.actor_step(*args)


def _assert_equal(st, m, step, names=TABLES + STATE + ('frames',)):
    torch.cuda.synchronize()
    want = m.tensors()
    for k in names:
        got = st[k].cpu()
        ref = torch.from_numpy(want[k]).view(got.shape)
        assert got.dtype == ref.dtype, k
        if not torch.equal(got, ref):
            bad = np.flatnonzero((got != ref).reshape(-1).numpy())
            pytest.fail('step %d: %s differs at %d element(s), first flat index %d: got %s, model %s'
                        % (step, k, bad.size, bad[0], got.reshape(-1)[bad[0]].item(), ref.reshape(-1)[bad[0]].item()))
    if 'ticket' in st:
        assert int(st['ticket']) == 0, 'step %d: the arrival ticket was not reset' % step


@pytest.mark.parametrize('case', AR.CASES, ids=AR.CASE_IDS)
def test_actor_step_equals_model_after_every_step(case):
    ext = _ext()
    m, q = AR.make_model(case)
    st = _upload(m, case[5])
    rolled = np.zeros(2, dtype=np.int64)
    for s in range(q.shape[0]):
        _actor_step(ext, st, q[s], AR.P_DONE)
        m.step(q[s])
        _assert_equal(st, m, s)
        rolled += [m.last_random.sum(), (~m.last_random).sum()]
        assert m.stale().size == 0
    eps = case[6]
    if eps == AR.EPS_RANDOM:
        assert rolled[1] == 0
    elif eps == AR.EPS_GREEDY:
        assert rolled[0] == 0
    elif case[0] in AR.BOTH_BRANCHES:
        assert rolled.min() > 0
    if case[7] == AR.BIG_CTR:
        assert int(st['rng'][1]) > 2 ** 32


@pytest.mark.parametrize('hw', [(4, 4), (4, 8)])
@pytest.mark.parametrize('K', [1, 2, 3, 4])
def test_gather_and_stack_paths_equal_model(K, hw):
    """``replay_gather_frames`` (with the per-sample columns riding along) over all live
    transitions and ``stack_states`` over the envs' stacks, after the device actor wrapped both
    rings, for every K the kernels are instantiated for."""
    from dist_dqn_amd.ops import kernels
    ext = _ext()
    C, E, A = 23, 3, 6
    case = ('gather_k%d_%dx%d' % ((K,) + hw), C, K, E, A, hw, [0.5, 0.5, 0.0], 0)
    m, q = AR.make_model(case)
    st = _upload(m, hw)
    for s in range(q.shape[0]):
        _actor_step(ext, st, q[s], AR.P_DONE)
        m.step(q[s])
    _assert_equal(st, m, q.shape[0] - 1)
    assert int(m.cursor[2]) == C
    live = m.live()
    idx = np.concatenate([live, live[::-1], live[::2]]).astype(np.int32)        # B = 58: more than one wave
    B = idx.size
    outs = [torch.full((B,), -1, dtype=torch.int32, device=DEV)] + [torch.full((B,), float('nan'), device=DEV)
                                                                    for _ in range(3)]
    s_d = torch.full((B, hw[0], hw[1], K), 0xEE, dtype=torch.uint8, device=DEV)
    ns_d = torch.full_like(s_d, 0xEE)
    kernels.replay_gather_frames(st['frames'], st['state_idx'], st['next_idx'], torch.from_numpy(idx).to(DEV),
                                 (s_d, ns_d), [st['actions'], st['rewards'], st['dones'], st['gammas']] + outs)
    torch.cuda.synchronize()
    s_ref, ns_ref = m.gather(idx)
    assert torch.equal(s_d.cpu().view(B, -1, K), torch.from_numpy(s_ref))
    assert torch.equal(ns_d.cpu().view(B, -1, K), torch.from_numpy(ns_ref))
    for o, col in zip(outs, (m.actions, m.rewards, m.dones, m.gammas)):
        assert torch.equal(o.cpu(), torch.from_numpy(col[idx]))
    # what the gather returns is what was recorded when each transition was written
    rec_s, rec_ns = m.recorded(idx)
    assert np.array_equal(s_ref, rec_s) and np.array_equal(ns_ref, rec_ns)
    out = torch.full((E, hw[0], hw[1], K), 0xEE, dtype=torch.uint8, device=DEV)
    ext.stack_states(st['frames'], st['stacks'], out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(E, -1, K), torch.from_numpy(m.stack_states()))


def _trees(m, P):
    """The consistent fp32 (sum, min) trees of the model's leaves (an empty leaf: 0 / +inf)."""
    s, _ = R.build_tree(m.leaves, P)
    _, mn = R.build_tree(np.where(m.leaf_set, m.leaves, np.float32(np.inf)), P)
    return s, mn


@pytest.mark.parametrize('C,E', [(23, 8), (24, 3), (64, 64)])
def test_per_insertion_at_running_max(C, E):
    """Prioritized replay: after every step the E new leaves hold the running max priority and
    the sum / min trees are the exact trees of their leaves -- also in the steps whose E slots
    straddle the wrap of C, and after priority updates moved the running max."""
    from dist_dqn_amd.replay.sumtree import DeviceSumTree
    ext = _ext()
    K, A, hw = 4, 6, (4, 4)
    m, q = AR.make_model(('per_c%d_e%d' % (C, E), C, K, E, A, hw, AR.EPS_RANDOM, 0), per=True)
    st = _upload(m, hw)
    tree = DeviceSumTree(C, DEV)
    P = tree.P
    assert P == m.per_P
    straddled = 0
    g = np.random.default_rng(C + E)
    for s in range(q.shape[0]):
        _actor_step(ext, st, q[s], AR.P_DONE, tree)
        m.step(q[s])
        _assert_equal(st, m, s)
        straddled += int((np.diff(m.last_t) < 0).any())
        leaves = tree.sum[P:].cpu().numpy()
        assert np.array_equal(leaves[m.last_t], np.full(E, m.max_p, dtype=np.float32)), s
        assert np.array_equal(leaves, m.leaves), s
        s_ref, m_ref = _trees(m, P)
        assert np.array_equal(tree.sum.cpu().numpy()[1:], s_ref[1:]), s
        assert np.array_equal(tree.min.cpu().numpy()[1:], m_ref[1:]), s
        assert float(tree.max_p) == float(m.max_p)
        if s % 3 == 1:
            # the learner's priority update between two actor steps: it moves leaves and (every
            # other time) the running max. Its values are this test's INPUT (powf on the device,
            # covered by the sum-tree tests): read back, they become the model's leaves.
            n = min(5, int(m.cursor[2]))
            idx = g.choice(int(m.cursor[2]), size=n, replace=False).astype(np.int32)
            td = g.uniform(0.1, 0.9, n).astype(np.float32) * (2.0 + s if s % 2 else 1.0)
            tree.update(torch.from_numpy(idx).to(DEV), torch.from_numpy(td).to(DEV), 0.6, 1e-6)
            torch.cuda.synchronize()
            m.leaves[idx] = tree.sum[P:].cpu().numpy()[idx]
            assert float(tree.max_p) >= float(m.max_p)
            m.max_p = np.float32(float(tree.max_p))
    assert (straddled > 0) == (C % E != 0)
    assert float(m.max_p) > 1.0


def _model_of(actor, rep, A):
    """A model that starts from the state a freshly built DeviceActor left on the device."""
    H, W = rep.obs_shape
    torch.cuda.synchronize()
    rng = actor.rng.cpu().tolist()
    return AR.ActorRingModel(rep.capacity, rep.num_frames, H * W, rep.k, actor.E, A, rng[0], actor.eps.cpu().numpy(),
                             actor.p_done, gamma=actor.gamma, ctr=rng[1],
                             frames=rep.frames.cpu().numpy().reshape(rep.num_frames, H * W),
                             stacks=actor.stacks.cpu().numpy(), cursor=rep.cursor.cpu().numpy())


def _replay_state(actor, rep):
    st = {k: getattr(rep, k) for k in TABLES + ('frames', 'cursor', 'size_dev')}
    st.update(stacks=actor.stacks, eps=actor.eps, rng=actor.rng, frames_done=actor.frames_done, ticket=actor.ticket)
    return st


@pytest.mark.parametrize('C,K,E', [(24, 4, 1), (23, 4, 2), (24, 4, 4), (23, 4, 8), (23, 1, 8), (24, 2, 3), (93, 3, 70)])
def test_ring_integrity_through_replay_and_actor(C, K, E):
    """``DeviceReplay`` + ``DeviceActor`` as a caller builds them (the actor sizes the replay's
    frame ring for its E envs), stepped by the stand-alone kernel on the replay's own tensors:
    after every step the gather of every live transition returns the bytes that transition's
    frames held when it was written. (On a ring of 2C + k + 8 frames this fails for E >= 2.)"""
    from dist_dqn_amd.actors.device_actor import DeviceActor
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.replay import DeviceReplay
    ext = _ext()
    A = 6
    cfg = preset('nature', 'Pong-v0', '--seed=0 --init_random_action_prob=1 --min_random_action_prob=1')
    rep = DeviceReplay(C, (4, 4), K, device=DEV)
    actor = DeviceActor(None, rep, cfg, num_envs=E, steps_per_call=1, seed=5, episode_len=1.0 / AR.P_DONE,
                        use_graph=False)
    assert rep.frames.shape[0] == rep.num_frames
    m = _model_of(actor, rep, A)
    st = _replay_state(actor, rep)
    q = np.zeros((E, A), dtype=np.float32)
    worst = 0
    for s in range(AR.num_steps(C, rep.num_frames, E)):
        _actor_step(ext, st, q, actor.p_done)
        m.step(q)
        _assert_equal(st, m, s)
        idx = torch.arange(rep.size(), dtype=torch.int32, device=DEV)
        got = rep.gather(idx)
        rec_s, rec_ns = m.recorded(m.live())
        ok_s = (got['states'].cpu().view(idx.numel(), -1, K) == torch.from_numpy(rec_s)).flatten(1).all(1)
        ok_n = (got['next_states'].cpu().view(idx.numel(), -1, K) == torch.from_numpy(rec_ns)).flatten(1).all(1)
        worst = max(worst, int((~(ok_s & ok_n)).sum()))
        assert np.array_equal(np.flatnonzero(~(ok_s & ok_n).numpy()), m.stale())
    print('C=%d K=%d E=%d F=%d: most live transitions with overwritten frames after a step: %d'
          % (C, K, E, rep.num_frames, worst))
    assert worst == 0


def test_fused_acting_equals_model():
    """The head kernel's acting blocks (``DeviceActor.step()`` -> ``act_fused``) on the Nature net:
    eps = eps_min = 1, so every action is the random one and nothing depends on Q (the greedy
    choice of this path is covered by its equality with the stand-alone kernel in
    test_executor_gpu.py). Tables, stacks, cursor, eps, rng, frames_done and the frames written
    in each step equal the model; at the end the whole ring does and no live transition is stale."""
    from dist_dqn_amd.actors.device_actor import DeviceActor
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    C, E, A = 64, 4, 6
    cfg = preset('nature', 'Pong-v0', '--seed=0 --backend=hip --dtype=bf16 --replay_memory_capacity=%d '
                 '--init_random_action_prob=1 --min_random_action_prob=1' % C)
    net = Network.create_network(cfg, (84, 84, 4), A, device=torch.device(DEV))
    rep = DeviceReplay(C, (84, 84), 4, device=DEV)
    actor = DeviceActor(net, rep, cfg, num_envs=E, steps_per_call=1, seed=11, episode_len=4, use_graph=False)
    assert getattr(net.executor, 'consumes_slots', False), 'not the fused acting path'
    m = _model_of(actor, rep, A)
    st = _replay_state(actor, rep)
    dones = 0
    for s in range(40):
        actor.step()
        m.step(None)
        _assert_equal(st, m, s, TABLES + STATE)
        sl = torch.from_numpy(m.last_slots).to(DEV)
        assert torch.equal(rep.frames[sl].cpu().view(sl.numel(), -1), torch.from_numpy(m.frames[m.last_slots])), s
        dones += int(m.dones[m.last_t].sum())
    assert dones > 0 and int(m.cursor[0]) == 40 * E % C and rep.size() == C
    _assert_equal(st, m, 39, ('frames',))
    assert m.stale(rep.frames.cpu().numpy()).size == 0 and m.stale().size == 0
