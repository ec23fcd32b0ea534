"""``--augment shift`` on the GPU: the gather-shift kernel (csrc/kernels/augment.hip) against the exact
Philox replica and a numpy shift, and the augmented learner step -- eager, in HIP graphs, and with
the device actors' step fused in -- against the torch executor fed the reference-augmented stacks.

Exactness: the shifts are integer arithmetic (Philox4x32-10 and a 32 x 32 -> 64 bit multiply) and the
stacks are byte copies, so both are compared bit for bit. The step's bounds are those of
tests/test_production_step_gpu.py for the same builds (per tensor: cosine > 0.985 and norm within
5 % for bf16, cosine > 0.9999 and norm within 0.2 % for fp32) and, for the loss, those of
tests/test_executor_gpu.py::test_loss_and_grad_match_oracle (3 % for the 16-bit builds, 1e-4 for fp32).
A conv1 forward or weight gradient that read the frame ring instead of the shifted stacks would see
unrelated pixels (the frames are uniform random bytes): every bound fails by a wide margin.
"""
import numpy as np
import pytest
import torch

import test_augment as ta

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SEED = ta.SEED
H = W = 84


def shift_np(x, dydx):
    """ta.shift_ref with whole-row indexing (checked against the loop in test_shift_np_is_the_loop)."""
    out = np.empty_like(x)
    for b in range(x.shape[0]):
        yi = np.clip(np.arange(x.shape[1]) + int(dydx[b, 0]), 0, x.shape[1] - 1)
        xi = np.clip(np.arange(x.shape[2]) + int(dydx[b, 1]), 0, x.shape[2] - 1)
        out[b] = x[b][yi][:, xi]
    return out


def edge_ctrs(B, pad):
    """The fewest counters from 0 upward (greedy, on the replica) after which +pad and -pad occurred on
    both axes and every dx mod 4 that [-pad, pad] holds occurred (pad = 1 has no dx = 2 mod 4): both edge
    paths, both row clamps, every byte alignment."""
    need = ({('y', -pad), ('y', pad), ('x', -pad), ('x', pad)}
            | {('r', d % 4) for d in range(-pad, pad + 1)})
    out = []
    for ctr in range(4000):
        sh = ta.shifts_ref(SEED, ctr, B, pad).reshape(-1, 2)
        have = ({('y', int(v)) for v in sh[:, 0]} | {('x', int(v)) for v in sh[:, 1]}
                | {('r', int(v) % 4) for v in sh[:, 1]}) & need
        if have:
            need -= have
            out.append(ctr)
        if not need:
            return out
    raise AssertionError('no covering counter set below 4000: %s' % need)


@pytest.fixture(scope='module')
def ring():
    """9 distinct random frames and, per B, slot tables that use every frame (the last one too)."""
    g = np.random.default_rng(9)
    frames = g.integers(0, 256, (9, H, W), dtype=np.uint8)
    tabs = {}
    for B in (3, 64):
        st = g.integers(0, 9, (B, 4)).astype(np.int32)
        nx = g.integers(0, 9, (B, 4)).astype(np.int32)
        st[0], nx[B - 1] = [8, 0, 8, 0], [0, 8, 8, 8]
        tabs[B] = (st, nx)
    return frames, tabs, torch.from_numpy(frames).to(DEV)


def _stack(frames, sl):
    return np.stack([frames[sl[:, c]] for c in range(4)], axis=-1)


def _run(frames_d, st, nx, ctr, pad):
    from dist_dqn_amd.ops import kernels
    c = torch.tensor([ctr], dtype=torch.int64, device=DEV)
    s, ns, sh = kernels.replay_gather_shift(frames_d, torch.from_numpy(st).to(DEV), torch.from_numpy(nx).to(DEV),
                                            SEED, c, pad)
    torch.cuda.synchronize()
    return s.cpu().numpy(), ns.cpu().numpy(), sh.cpu().numpy()


def test_shift_np_is_the_loop():
    g = np.random.default_rng(1)
    x = g.integers(0, 256, (3, H, W, 4), dtype=np.uint8)
    d = np.array([[-16, 16], [3, -5], [0, 1]])
    assert np.array_equal(shift_np(x, d), ta.shift_ref(x, d))


@pytest.mark.parametrize('B', [3, 64])
@pytest.mark.parametrize('pad', [1, 4, 16])
def test_kernel_shifts_and_stacks_equal_the_reference(ring, B, pad):
    frames, tabs, frames_d = ring
    st, nx = tabs[B]
    s0, n0 = _stack(frames, st), _stack(frames, nx)
    cover = edge_ctrs(B, pad)
    assert len(cover) <= 8
    for ctr in cover + [2 ** 32 + 5, 2 ** 40 + 2 ** 32 - 1, 2 ** 62 + 1]:
        s, ns, sh = _run(frames_d, st, nx, ctr, pad)
        want = ta.shifts_ref(SEED, ctr, B, pad)
        assert sh.dtype == np.int32 and np.array_equal(sh, want), (ctr, sh[:2], want[:2])
        assert np.array_equal(s, shift_np(s0, want[:, 0])), ('s', ctr)
        assert np.array_equal(ns, shift_np(n0, want[:, 1])), ('ns', ctr)
    # the high counter words matter: ctr and ctr + 2^32 draw different sets
    assert not np.array_equal(ta.shifts_ref(SEED, 5, B, pad), ta.shifts_ref(SEED, 2 ** 32 + 5, B, pad))


@pytest.mark.parametrize('B', [3, 64])
def test_pad_zero_is_the_plain_gather(ring, B):
    """pad = 0 == replay_gather_frames on the transitions whose slots the tables hold."""
    from dist_dqn_amd.ops import kernels
    frames, tabs, frames_d = ring
    st, nx = tabs[B]
    # replay_gather_frames forms s' from the state's last three slots + next_idx
    nx = np.concatenate([st[:, 1:], nx[:, 3:]], axis=1).astype(np.int32)
    s, ns, sh = _run(frames_d, st, nx, 123, 0)
    assert not sh.any()
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    gs, gns = kernels.replay_gather_frames(frames_d, torch.from_numpy(st).to(DEV),
                                           torch.from_numpy(np.ascontiguousarray(nx[:, 3])).to(DEV), idx)
    torch.cuda.synchronize()
    assert np.array_equal(s, gs.cpu().numpy()) and np.array_equal(ns, gns.cpu().numpy())


# ------------------------------------------------------------------------ the step
CAP = 4096
STEP_CASES = {                       # (preset, dtype, extra flags)
    'nature-bf16': ('nature', 'bf16', ''),
    'nature-fp32': ('nature', 'fp32', ''),
    'cnn-bf16': ('atari', 'bf16', ''),
    'nature-bf16-det': ('nature', 'bf16', '--det_wgrad=1'),      # conv1 partials summed by the optimizer launch
}


def _build(env_type, dtype, extra, B=4, acting=False, use_graph=False, augment=True, fill=CAP):
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    cfg = preset(env_type, 'Pong-v0', '--seed=0 --backend=hip --dtype=%s --replay_memory_capacity=%d --lr=0.01 '
                 '--minibatch_size=%d %s %s' % (dtype, CAP, B, '--augment=shift' if augment else '', extra))
    net = Network.create_network(cfg, (84, 84, 4), 6, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    net.online.flat.normal_(0.0, 0.03, generator=g)      # every layer carries signal
    net.target.flat.normal_(0.0, 0.03, generator=g)
    net.refresh_packed()
    rep = DeviceReplay(CAP, (84, 84), 4, device=DEV, seed=3)
    rep.fill_synthetic(fill, 6, seed=3)
    actor = None
    if acting:
        from dist_dqn_amd.actors.device_actor import DeviceActor
        actor = DeviceActor(net, rep, cfg, num_envs=4, steps_per_call=1, seed=11)
        assert actor.can_fuse(B)
    return cfg, net, rep, Learner(net, rep, cfg, use_graph=use_graph, actor=actor)


@pytest.mark.parametrize('case', sorted(STEP_CASES))
def test_augmented_step_matches_the_oracle_on_shifted_stacks(case):
    """One augmented SGD step at B = 4, as the CLI runs it (fold, fused weight-gradient + optimizer
    launch where the build has it, minibatch drawn by the previous optimizer launch): the loss and the
    gradient the update applied (recovered from the RMSProp update as in test_production_step_gpu.py)
    against the torch executor on the numpy-shifted stacks of the same minibatch."""
    from dist_dqn_amd.models.executor import TorchExecutor
    from dist_dqn_amd.ops import augment
    env_type, dtype, extra = STEP_CASES[case]
    cfg, net, rep, ln = _build(env_type, dtype, extra)
    B = cfg.minibatch_size
    ln.step()
    torch.cuda.synchronize()
    assert ln._sample_mode() == 'opt' and ln._presampled
    assert ln._det_wgrad == ('det' in case)
    step = int(net.global_step)
    assert step == 1
    sb = rep.slot_batch(B)
    batch = {k: v.clone() for k, v in rep.gather(sb['idx'].clone()).items()}
    want = ta.shifts_ref(augment.aug_seed(0, 0), step, B, cfg.aug_pad)
    assert np.abs(want).max() > 0
    batch['states'] = torch.from_numpy(shift_np(batch['states'].cpu().numpy(), want[:, 0])).to(DEV)
    batch['next_states'] = torch.from_numpy(shift_np(batch['next_states'].cpu().numpy(), want[:, 1])).to(DEV)
    w0, tgt0 = net.online.flat.clone(), net.target.flat.clone()
    loss = float(ln.step())
    torch.cuda.synchronize()
    assert np.array_equal(ln.aug_shifts.cpu().numpy(), want)
    opt, lay = net.optimizer, net.layout
    reg = torch.zeros_like(w0)
    reg[:lay.reg_end] = float(cfg.reg_param)
    g_rec = (w0 - net.online.flat).double() * torch.sqrt(opt.slots[0].double() + float(opt.hp['rms_eps'])) / float(opt.lr)
    g_rec = (g_rec - reg.double() * w0.double()).float()
    oracle = TorchExecutor(net.arch, lay, input_scale=cfg.input_scale, loss=cfg.loss, oracle=True,
                           huber_delta=cfg.huber_delta, double_dqn=cfg.double_dqn)
    g_ref = torch.zeros_like(w0)
    loss_r, _ = oracle.loss_and_grad(w0, tgt0, batch, g_ref, None, None)
    torch.cuda.synchronize()
    loss_r = float(loss_r)
    tol = (0.9999, 2e-3, 1e-4) if dtype == 'fp32' else (0.985, 0.05, 3e-2)
    figs = []
    for name in lay.names:
        o, k = lay.offsets[name], lay.numel(name)
        a, b = g_rec[o:o + k].double(), g_ref[o:o + k].double()
        if float(b.norm()) == 0.0:
            continue
        figs.append((name, float(torch.nn.functional.cosine_similarity(a, b, dim=0)), float(a.norm() / b.norm())))
    print(case, 'loss %.6g oracle %.6g' % (loss, loss_r), figs)
    assert abs(loss - loss_r) / abs(loss_r) < tol[2], (case, loss, loss_r)
    for name, cos, ratio in figs:
        assert cos > tol[0] and abs(ratio - 1.0) < tol[1], (case, name, cos, ratio)
    names = [f[0] for f in figs]
    assert len(names) >= 10 and 'conv1/w' in names and 'conv1/b' in names, names


def test_step_many_graph_draws_fresh_shifts_per_step():
    """A graph of 3 step bodies replayed from global_step 0: the three bodies' shift sets are the
    reference's at global_step 0, 1 and 2, all different."""
    from dist_dqn_amd.ops import augment
    cfg, net, rep, ln = _build('nature', 'bf16', '', use_graph=True)
    for _ in range(3):                       # eager warm-up + the one-step capture
        ln.step()
    torch.cuda.synchronize()
    assert ln.can_step_many()
    net.global_step.zero_()
    ln.aug_shift_log.zero_()
    first = ln._aug_calls
    ln.step_many(3)
    torch.cuda.synchronize()
    assert int(net.global_step) == 3
    log = ln.aug_shift_log.cpu().numpy()
    sets = [log[(first + i) % 8] for i in range(3)]
    for i, sh in enumerate(sets):
        assert np.array_equal(sh, ta.shifts_ref(augment.aug_seed(0, 0), i, cfg.minibatch_size, cfg.aug_pad)), i
    assert not np.array_equal(sets[0], sets[1]) and not np.array_equal(sets[1], sets[2])
    assert not np.array_equal(sets[0], sets[2])
    # a second replay goes on from global_step 3
    ln.step_many(3)
    torch.cuda.synchronize()
    log = ln.aug_shift_log.cpu().numpy()
    assert np.array_equal(log[(first + 2) % 8], ta.shifts_ref(augment.aug_seed(0, 0), 5, cfg.minibatch_size, cfg.aug_pad))


def test_augmented_graph_equals_eager():
    """tests/test_executor_gpu.py::test_learner_step_graph_equals_eager with --augment shift, its
    tolerance (conv weight gradients combine M-chunks with fp32 atomics), on the loss too."""
    outs = []
    for graph in (False, True):
        cfg, net, rep, ln = _build('nature', 'bf16', '', use_graph=graph)
        for _ in range(6):
            loss = ln.step()
        torch.cuda.synchronize()
        assert int(net.global_step) == 6 and (ln._graphs is not None) == graph
        outs.append((net.online.flat.clone(), loss.clone(), ln.aug_shifts.clone()))
    assert torch.equal(outs[0][2], outs[1][2])
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-6)


def test_fused_acting_is_unshifted():
    """--device_envs style step (E = 4 device actors fused into the learner's launches, B = 8), first
    step from equal weights with and without --augment shift: the actors read the ring unshifted, so
    their actions and everything they appended are bit-equal; the learner's loss differs."""
    runs = []
    for aug in (False, True):
        torch.manual_seed(17)                  # (DeviceActor draws the envs' reset frames from torch's generator)
        cfg, net, rep, ln = _build('nature', 'bf16', '', B=8, acting=True, augment=aug, fill=CAP // 2)
        assert ln.actor is not None, 'acting is fused into the learner launches'
        loss = float(ln.step())
        torch.cuda.synchronize()
        a = ln.actor
        runs.append((loss, [t.clone() for t in (rep.actions, rep.rewards, rep.dones, rep.gammas, rep.state_idx,
                                                rep.next_idx, rep.frames, rep.cursor, rep.size_dev, a.stacks, a.rng,
                                                a.eps, a.frames_done)]))
        assert int(rep.cursor[0]) == CAP // 2 + 4, 'four transitions appended'
    for x, y in zip(runs[0][1], runs[1][1]):
        assert torch.equal(x, y)
    assert runs[0][0] != runs[1][0]
