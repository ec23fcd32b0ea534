"""Global gradient-norm clipping (``--max_grad_norm``) off the GPU: the flag and its refusals, the torch
form of the clip against a float64 loop, a clipped TorchExecutor step, a short CartPole run, two gloo
ranks that stay bit-equal, and the ``grad_norm`` summary scalar.

    norm  = grad_scale * ||g||_2   (g: the whole flat loss gradient, before the decoupled L2 term)
    scale = C / max(norm, C)       (exactly 1 when norm <= C; 0 when the norm is not finite)
    g    <- g * scale
"""
import glob
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ------------------------------------------------------------------ the flag
def test_flag_default_and_parsing():
    from dist_dqn_amd.config import Config, defaults, flag_names, parse_args, preset
    assert defaults().max_grad_norm == 0.0 and Config().max_grad_norm == 0.0
    assert 'max_grad_norm' in flag_names()
    c = parse_args(['--max_grad_norm', '10'])
    assert c.max_grad_norm == 10.0 and isinstance(c.max_grad_norm, float)
    assert parse_args(['--max_grad_norm=0.5']).max_grad_norm == 0.5
    assert parse_args(['--max_grad_norm=0', '--async_ps']).max_grad_norm == 0.0     # (off: nothing to refuse)
    # presets are not changed
    for kind, env in (('nature', 'Pong-v0'), ('atari', 'Pong-v0'), ('control', 'CartPole-v0')):
        assert preset(kind, env).max_grad_norm == 0.0
    assert preset('nature', 'Pong-v0', '--max_grad_norm 40').max_grad_norm == 40.0


def test_negative_norm_is_refused(capsys):
    from dist_dqn_amd.config import parse_args
    with pytest.raises(SystemExit):
        parse_args(['--max_grad_norm=-1'])
    assert '--max_grad_norm must be >= 0' in capsys.readouterr().err


def test_async_ps_is_refused(capsys):
    from dist_dqn_amd.config import parse_args
    with pytest.raises(SystemExit):
        parse_args(['--max_grad_norm=10', '--async_ps'])
    err = capsys.readouterr().err
    assert '--max_grad_norm and --async_ps cannot be combined' in err
    assert 'arrival order' in err and 'on the server' in err


def test_kernel_tuning_help_names_every_key():
    import dataclasses

    from dist_dqn_amd.config import build_parser
    from dist_dqn_amd.ops.tuning import KernelTuning
    text = ' '.join(build_parser().format_help().split())
    for f in dataclasses.fields(KernelTuning):
        assert f.name in text, f.name


# ------------------------------------------------------------------ the formula
def _loop64(x, C, grad_scale=1.0):
    """The clip in a float64 python loop on the fp32 values."""
    s = 0.0
    for v in x.tolist():
        s += v * v
    norm = math.sqrt(s) * grad_scale
    if not math.isfinite(norm):
        return norm, 0.0
    return norm, C / max(norm, C)


@pytest.mark.parametrize('n', [1, 7, 1000])
@pytest.mark.parametrize('rel', [0.5, 2.0, 10.0])          # C / norm: clipping active, inactive
@pytest.mark.parametrize('grad_scale', [1.0, 0.125])
def test_torch_formula_matches_float64_loop(n, rel, grad_scale):
    from dist_dqn_amd.ops import kernels
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3.0
    norm0, _ = _loop64(x, 1.0, grad_scale)
    C = float(np.float32(rel * norm0))
    norm, scale = _loop64(x, C, grad_scale)
    y, stats = x.clone(), torch.zeros(2)
    kernels.grad_clip(y, C, grad_scale, stats)
    # float64 accumulation, one rounding to fp32, one fp32 product: a few units of 2^-24
    assert abs(float(stats[0]) - norm) <= 4 * 2.0 ** -24 * norm
    assert abs(float(stats[1]) - scale) <= 8 * 2.0 ** -24 * scale
    if rel > 1.0:
        assert float(stats[1]) == 1.0 and torch.equal(y, x)          # the same bits
    else:
        assert torch.equal(y, x * stats[1])
        assert abs(float(y.double().norm()) * grad_scale - C) <= 1e-5 * C


def test_norm_equal_to_the_bound_is_not_clipped():
    from dist_dqn_amd.ops import kernels
    x = torch.tensor([3.0, 0.0, 4.0])
    y, stats = x.clone(), torch.zeros(2)
    kernels.grad_clip(y, 5.0, 1.0, stats)
    assert stats.tolist() == [5.0, 1.0] and torch.equal(y, x)
    kernels.grad_clip(y, 2.5, 0.5, stats)                     # (the effective gradient has norm 2.5)
    assert stats.tolist() == [2.5, 1.0] and torch.equal(y, x)
    kernels.grad_clip(y, 2.5, 1.0, stats)
    assert stats.tolist() == [5.0, 0.5] and torch.equal(y, x * 0.5)


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), -float('inf')])
def test_non_finite_gradient_gives_scale_zero(bad):
    from dist_dqn_amd.ops import kernels
    x = torch.randn(100, generator=torch.Generator().manual_seed(0))
    x[37] = bad
    stats = torch.zeros(2)
    kernels.grad_clip(x, 10.0, 1.0, stats)
    assert not math.isfinite(float(stats[0])), 'the norm is reported as computed'
    assert float(stats[1]) == 0.0 and torch.equal(x, torch.zeros(100))


def test_bad_max_norm_is_refused():
    from dist_dqn_amd.ops import kernels
    for c in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='max_norm'):
            kernels.grad_clip(torch.ones(4), c, 1.0, torch.zeros(2))


# ------------------------------------------------------------------ a TorchExecutor step
def _simple(extra=()):
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.models.network import Network
    cfg = parse_args(['--device=cpu', '--seed=1', '--network=simple', '--optimizer=sgd', '--lr=0.5',
                      '--reg_param=0.01'] + list(extra))
    return cfg, Network.create_network(cfg, (4,), 2)


def _batch(seed=3, n=16):
    g = torch.Generator().manual_seed(seed)
    return {'states': torch.randn(n, 4, generator=g), 'next_states': torch.randn(n, 4, generator=g),
            'actions': torch.randint(0, 2, (n,), generator=g), 'rewards': torch.randn(n, generator=g) * 5.0,
            'dones': (torch.rand(n, generator=g) < 0.3).float(), 'gammas': torch.full((n,), 0.9)}


def _applied(net, w0, cfg):
    """SGD: w' = w - lr (g + reg w) on the regularised range, so g = (w - w') / lr - reg w."""
    reg = torch.zeros_like(w0)
    reg[:net.layout.reg_end] = float(cfg.reg_param)
    return (w0.double() - net.online.flat.double()) / float(cfg.lr) - reg.double() * w0.double()


def test_torch_executor_step_is_clipped_to_the_bound_and_keeps_its_direction():
    batch = _batch()
    cfg0, ref = _simple()
    assert ref.executor.name == 'torch' and ref.grad_norm is None
    w0 = ref.online.flat.clone()
    ref.train_step(batch)
    g0 = _applied(ref, w0, cfg0)
    n0 = float(g0.norm())
    assert n0 > 0.0 and ref.grad_norm is None, 'an unclipped run allocates and reports nothing'
    # clipping active: the applied loss gradient has norm C and the unclipped direction; the L2 term
    # is not clipped (it is subtracted whole in _applied)
    C = 0.5 * n0
    cfg, net = _simple(['--max_grad_norm=%r' % C])
    assert torch.equal(net.online.flat, w0)
    net.train_step(batch)
    g = _applied(net, w0, cfg)
    assert abs(float(net.grad_norm) - n0) <= 1e-5 * n0, 'grad_norm is the pre-clip norm'
    assert abs(float(g.norm()) - C) <= 1e-4 * C
    assert float(torch.nn.functional.cosine_similarity(g, g0, dim=0)) > 1.0 - 1e-6
    torch.testing.assert_close(g, g0 * 0.5, rtol=1e-3, atol=1e-5 * n0)
    # clipping inactive: bit for bit the unclipped step
    cfg, net = _simple(['--max_grad_norm=%r' % (10.0 * n0)])
    net.train_step(batch)
    assert torch.equal(net.online.flat, ref.online.flat)
    assert abs(float(net.grad_norm) - n0) <= 1e-5 * n0


def test_learner_step_clips_on_the_cpu_for_simple_and_cnn():
    """The Learner's step (device replay, torch executor) goes through Network.clip_grads for the
    `simple` MLP and the reference `cnn`: the recorded norm is that of the gradient the step computed,
    and the buffer the optimizer read has norm C."""
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    cfg = parse_args(['--device=cpu', '--seed=5', '--network=cnn', '--optimizer=rmsprop', '--minibatch_size=4',
                      '--replay_memory_capacity=64', '--max_grad_norm=1e-3'])
    net = Network.create_network(cfg, (84, 84, 4), 6)
    rep = DeviceReplay(64, (84, 84), 4, device='cpu', seed=0)
    rep.fill_synthetic(64, 6, seed=0, episode_len=16)
    ln = Learner(net, rep, cfg)
    assert not ln._defer_fc and not ln._defer_wgrad and not ln._det_wgrad and not ln._dp_fused
    ln.step()
    assert float(ln.grad_norm) > 1e-3, 'this gradient is larger than the bound'
    assert abs(float(net.grad.double().norm()) - 1e-3) <= 1e-5 * 1e-3
    assert Learner(net, rep, cfg.replace(max_grad_norm=0.0)).grad_norm is None


# ------------------------------------------------------------------ a short run
def test_cartpole_still_learns_with_clipping(tmp_path):
    """tests/test_agent_ckpt.py::test_cartpole_learns's run and criterion with --max_grad_norm 10; the
    event file carries a grad_norm scalar beside each loss scalar."""
    from dist_dqn_amd.cli import run_worker
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.utils.metrics import read_tfrecords
    cfg = parse_args(['--env=CartPole-v0', '--network=simple', '--optimizer=adam', '--lr=0.002',
                      '--minibatch_size=64', '--num_episodes=400', '--max_steps_per_episode=200',
                      '--replay_memory_capacity=20000', '--target_update_freq=200', '--reward_discount=0.99',
                      '--init_random_action_prob=1.0', '--min_random_action_prob=0.02',
                      '--random_action_explore_steps=4000', '--logdir=%s' % tmp_path, '--seed=4',
                      '--max_train_steps=15000', '--reg_param=0', '--device=cpu', '--checkpoint_secs=0',
                      '--max_grad_norm=10'])
    agent = run_worker(cfg)
    rewards = list(agent.stats.rewards)
    early = [r['mean100'] for r in map(json.loads, open(os.path.join(tmp_path, 'metrics.rank0.jsonl')))
             if r.get('kind') == 'episode'][20]
    print('last-30 mean %.1f, early mean100 %.1f' % (np.mean(rewards[-30:]), early))
    assert np.mean(rewards[-30:]) > 60 and np.mean(rewards[-30:]) > 2 * early
    recs = [r for p in glob.glob(os.path.join(tmp_path, 'events.out.tfevents.*')) for r in read_tfrecords(p)]
    n_loss = sum(1 for r in recs if b'loss' in r)
    n_norm = sum(1 for r in recs if b'grad_norm' in r)
    assert n_norm == n_loss > 10, (n_norm, n_loss)


def test_no_grad_norm_scalar_without_the_flag(tmp_path):
    from dist_dqn_amd.agent import DQNAgent
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.envs import CartPoleEnv
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import ReplayMemory
    from dist_dqn_amd.utils.metrics import read_tfrecords
    counts = {}
    for flag in ('0', '10'):
        d = tmp_path / flag
        cfg = parse_args(['--device=cpu', '--seed=0', '--logdir=%s' % d, '--network=simple', '--optimizer=adam',
                          '--minibatch_size=16', '--replay_start_size=32', '--summary_freq=10',
                          '--max_train_steps=60', '--max_grad_norm=' + flag])
        net = Network.create_network(cfg, (4,), 2)
        DQNAgent(CartPoleEnv(seed=0), net, None, ReplayMemory(2000), cfg).train(20, 50)
        recs = [r for p in glob.glob(os.path.join(d, 'events.out.tfevents.*')) for r in read_tfrecords(p)]
        counts[flag] = (sum(1 for r in recs if b'loss' in r), sum(1 for r in recs if b'grad_norm' in r))
    assert counts['0'][0] > 0 and counts['0'][1] == 0, counts
    assert counts['10'][1] == counts['10'][0] > 0, counts


# ------------------------------------------------------------------ two ranks
def _worker_clipped(rank, world, port, tmpdir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.parallel import broadcast_flat, check_replicas_equal, init_distributed
    from dist_dqn_amd.replay import DeviceReplay
    cfg = parse_args(['--device=cpu', '--seed=5', '--network=cnn', '--optimizer=rmsprop', '--minibatch_size=4',
                      '--target_update_freq=2', '--replay_memory_capacity=64', '--max_grad_norm=1e-3'])
    ctx = init_distributed(cfg, device='cpu')
    net = Network.create_network(cfg, (84, 84, 4), 6)
    broadcast_flat(ctx, net.online.flat)
    net.target.copy_from(net.online)
    rep = DeviceReplay(64, (84, 84), 4, device='cpu', seed=rank)
    rep.fill_synthetic(64, 6, seed=rank, episode_len=16)    # different data per rank
    ln = Learner(net, rep, cfg, ctx)
    clipped = 0
    for _ in range(20):
        ln.step()
        clipped += float(net._clip_stats[1]) < 1.0
        # the norm is that of the AVERAGED gradient: the same bits on both ranks
        norms = [torch.zeros(1) for _ in range(world)]
        dist.all_gather(norms, ln.grad_norm.view(1).clone())
        assert all(torch.equal(norms[0], t) for t in norms), norms
    assert clipped > 0, 'no step of this run was clipped'
    assert check_replicas_equal(ctx, net.online.flat)
    assert check_replicas_equal(ctx, net.target.flat)
    assert int(net.global_step) == 20 and ln.train_steps == 20
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_stay_bit_equal_over_20_clipped_steps(tmp_path):
    mp.spawn(_worker_clipped, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
