"""The shipped graph step with ``--max_grad_norm`` against ``TorchExecutor(oracle=True)``, built as
tests/test_production_step_gpu.py builds it (small replays, B = 8).

Each case first measures N0, the norm of the oracle's gradient of the step after four warm-up steps of
an unclipped learner, then runs the learner with C = 0.5 N0 (clipping active) and C = 10 N0
(inactive). The gradient the checked step applied is recovered from the optimizer update as that file
recovers it (RMSProp: g = (w - w') sqrt(ms' + eps) / lr; Adam: g = (m' - b1 m) / (1 - b1); minus the
decoupled L2 term, which is not clipped) and compared per tensor with the oracle's gradient of the same
minibatch / weights / noise, clipped by the torch form of the formula: that file's thresholds, fp32
cosine > 0.9999 and norm within 0.2 %, 16-bit cosine > 0.985 and norm within 5 %; the 16-bit norm margin
also holds ``learner.grad_norm`` to the oracle's norm. (RMSProp and Adam steps barely depend on the
gradient's scale, so the checked step's own oracle norm N stays close to N0 whether the warm-up steps
were clipped or not; the test asserts on which side of C it lies before it relies on it.)

Also here: graph step == eager step, ``step_many(4)`` == four single steps (tests/test_qr_step_gpu.py's
tolerance), and the launch sequences: unchanged with the flag off, exactly the clip launches more than
the unfused step with it on (tests/launch_trace.py).
"""
import os

import pytest
import torch

import launch_trace as lt

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CAP = 4096
RAINBOW = '--dueling --double_dqn --distributional --noisy --prioritized_replay --optimizer=adam'
# name -> (preset, dtype, flags)
CASES = {
    'nature_bf16': ('nature', 'bf16', ''),
    'nature_dd_fp32': ('nature', 'fp32', '--dueling --double_dqn --loss=huber'),
    'rainbow_fp16': ('nature', 'fp16', RAINBOW),          # noisy + PER + C51: sigma gradients in the norm
    'cnn_fp32': ('atari', 'fp32', ''),                    # the reference's `cnn`
    'qr_bf16': ('nature', 'bf16', '--quantile --dueling --double_dqn'),
    'munchausen_bf16': ('nature', 'bf16', '--munchausen --loss=huber'),
}


def _build(case, clip, use_graph=True, seed=0, spread=True, extra=''):
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    pre, dtype, flags = CASES[case]
    lr = 0.0001 if 'adam' in flags else 0.01
    cfg = preset(pre, 'Pong-v0', '--seed=%d --backend=hip --dtype=%s --replay_memory_capacity=%d --lr=%g '
                 '--minibatch_size=8 --max_grad_norm=%r %s %s' % (seed, dtype, CAP, lr, float(clip), flags, extra))
    net = Network.create_network(cfg, (84, 84, 4), 6, device=DEV)
    assert net.executor.name == 'hip'
    if spread:                                     # every layer carries signal
        g = torch.Generator(device=DEV).manual_seed(7)
        net.online.flat.normal_(0.0, 0.03, generator=g)
        net.target.flat.normal_(0.0, 0.03, generator=g)
        net.refresh_packed()
    rep = DeviceReplay(CAP, (84, 84), 4, device=DEV, prioritized=cfg.prioritized_replay, seed=3)
    rep.fill_synthetic(CAP, 6, seed=3)
    return cfg, net, rep, Learner(net, rep, cfg, use_graph=use_graph)


def _oracle(cfg, net):
    from dist_dqn_amd.models.executor import TorchExecutor
    kw = {}
    if cfg.munchausen:
        kw['munchausen'] = (cfg.m_alpha, cfg.m_tau, cfg.m_clip)
    else:
        kw['double_dqn'] = cfg.double_dqn
    return TorchExecutor(net.arch, net.layout, input_scale=cfg.input_scale, loss=cfg.loss, oracle=True,
                         huber_delta=cfg.huber_delta, **kw)


def _checked_step(cfg, net, rep, ln):
    """Four steps (eager warm-up, capture, replays), then one more: (gradient recovered from that
    step's update, the oracle's unclipped gradient of the same step)."""
    for _ in range(4):
        ln.step()
    torch.cuda.synchronize()
    assert ln._graphs is not None, 'the shipped step runs as a HIP graph'
    assert ln._sample_mode() == 'opt' and ln._presampled, 'next minibatch drawn by the optimizer launch'
    sb = rep.slot_batch(cfg.minibatch_size)
    batch = {k: v.clone() for k, v in rep.gather(sb['idx'].clone()).items()}
    if 'weights' in sb:
        batch['weights'] = sb['weights'].clone()
    w0, tgt0 = net.online.flat.clone(), net.target.flat.clone()
    s0 = [s.clone() for s in net.optimizer.slots]
    noise = net.noise.clone() if getattr(net, 'noise', None) is not None else None
    tnoise = net.noise_target.clone() if getattr(net, 'noise_target', None) is not None else None
    ln.step()
    torch.cuda.synchronize()
    assert not torch.equal(net.online.flat, w0)
    opt, lay = net.optimizer, net.layout
    reg = torch.zeros_like(w0)
    reg[:lay.reg_end] = float(cfg.reg_param)
    if cfg.optimizer == 'rmsprop':
        g_rec = (w0 - net.online.flat).double() * torch.sqrt(opt.slots[0].double() + float(opt.hp['rms_eps'])) / float(opt.lr)
    else:
        assert cfg.optimizer == 'adam'
        b1 = float(opt.hp['b1'])
        g_rec = (opt.slots[0].double() - b1 * s0[0].double()) / (1.0 - b1)
    g_rec = (g_rec - reg.double() * w0.double()).float()
    g_ref = torch.zeros_like(w0)
    _oracle(cfg, net).loss_and_grad(w0, tgt0, batch, g_ref, noise, tnoise)
    torch.cuda.synchronize()
    return g_rec, g_ref


def _compare(case, what, lay, g_rec, g_want, dtype):
    tol = (0.9999, 2e-3) if dtype == 'fp32' else (0.985, 0.05)
    checked, worst = [], (2.0, 0.0)
    for name in lay.names:
        o, k = lay.offsets[name], lay.numel(name)
        a, b = g_rec[o:o + k].double(), g_want[o:o + k].double()
        if float(b.norm()) == 0.0:
            continue
        cos = float(torch.nn.functional.cosine_similarity(a, b, dim=0))
        ratio = float(a.norm() / b.norm())
        worst = (min(worst[0], cos), max(worst[1], abs(ratio - 1.0)))
        assert cos > tol[0] and abs(ratio - 1.0) < tol[1], (case, what, name, cos, ratio)
        checked.append(name)
    print('%s %s: worst cosine %.6f, worst |norm ratio - 1| %.3g over %d tensors'
          % (case, what, worst[0], worst[1], len(checked)))
    assert len(checked) >= 10, checked
    if 'noisy' in CASES[case][2]:
        assert any(n.endswith('w_sigma') for n in checked) and any(n.endswith('b_sigma') for n in checked), checked


@pytest.mark.parametrize('case', sorted(CASES))
def test_clipped_graph_step_matches_the_clipped_oracle_every_tensor(case):
    from dist_dqn_amd.ops import kernels
    dtype = CASES[case][1]
    margin = 2e-3 if dtype == 'fp32' else 0.05
    # ---- N0: the oracle's unclipped norm at the checked step of an unclipped learner
    cfg, net, rep, ln = _build(case, 0.0)
    assert ln.grad_norm is None and net.grad_norm is None and not hasattr(net, '_clip_stats')
    _, g_ref = _checked_step(cfg, net, rep, ln)
    N0 = float(g_ref.double().norm())
    assert N0 > 0.0
    del ln, net, rep
    for rel in (0.5, 10.0):
        C = rel * N0
        cfg, net, rep, ln = _build(case, C)
        assert not ln._defer_fc and not ln._defer_wgrad and not ln._det_wgrad and not ln._dp_fused
        g_rec, g_ref = _checked_step(cfg, net, rep, ln)
        N = float(g_ref.double().norm())
        gn = float(ln.grad_norm)
        scale = float(net._clip_stats[1])
        print('%s C = %.2f N0: N0 %.6g, oracle norm %.6g, learner.grad_norm %.6g, scale %.6g, recovered norm %.6g'
              % (case, rel, N0, N, gn, scale, float(g_rec.double().norm())))
        assert abs(gn - N) <= margin * N, (case, rel, gn, N)
        g_want, stats = g_ref.clone(), torch.zeros(2, device=DEV)
        kernels.grad_clip(g_want, C, 1.0, stats, backend='torch')
        if rel < 1.0:
            assert N * (1.0 - margin) > C, 'this step must be clipped for the check to mean anything'
            assert scale < 1.0
            assert abs(float(g_rec.double().norm()) - C) <= margin * C, (case, float(g_rec.double().norm()), C)
            assert abs(float(g_want.double().norm()) - C) <= 1e-5 * C
        else:
            assert N * (1.0 + margin) < C and scale == 1.0 and torch.equal(g_want, g_ref)
        _compare(case, 'C = %.1f N0' % rel, net.layout, g_rec, g_want, dtype)
        del ln, net, rep


@pytest.mark.parametrize('case', ['nature_bf16', 'nature_dd_fp32'])
def test_clipped_graph_step_equals_eager_step(case):
    outs = []
    for graph in (False, True):
        _, net, _, ln = _build(case, 0.05, use_graph=graph, seed=3, spread=False)
        for _ in range(4):                     # (graph: eager warm-up, capture, then one replayed step)
            ln.step()
        torch.cuda.synchronize()
        assert int(net.global_step) == 4 and (ln._graphs is not None) == graph
        assert 0.0 < float(net._clip_stats[1]) <= 1.0
        outs.append((net.online.flat.clone(), net._clip_stats.clone()))
    # wgrad combines M-chunks with fp32 atomics (order-dependent last bits)
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-6)


def test_clipped_step_many_equals_single_steps():
    outs = []
    for many in (False, True):
        _, net, _, ln = _build('nature_bf16', 0.05, seed=3, spread=False, extra='--target_update_freq=5')
        for _ in range(3):                     # eager warm-up + the single-step capture
            ln.step()
        if many:
            assert ln.can_step_many()
            ln.step_many(4)
        else:
            for _ in range(4):
                ln.step()
        torch.cuda.synchronize()
        assert int(net.global_step) == 7 and ln.train_steps == 7
        outs.append((net.online.flat.clone(), net.target.flat.clone(), net._clip_stats.clone()))
    # (conv weight gradients combine M-chunks with fp32 atomics: order-dependent last bits)
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


def _names(calls):
    return [c[0] for c in calls]


def test_flag_off_plans_and_launches_what_the_flagship_does(monkeypatch):
    """--max_grad_norm=0 spelled out: the flagship's planned flags, its golden launch trace argument by
    argument, no clip launch and no clip buffer."""
    monkeypatch.setitem(lt.CONFIGS, 'clip_off', ('nature', '--dtype=bf16 --max_grad_norm=0', {}))
    got = lt.dumps(lt.record_steps('clip_off'))
    with open(os.path.join(lt.GOLDEN_DIR, 'nature_bf16.json')) as f:
        assert got == f.read()
    assert 'grad_clip' not in got
    cfg, net, rep, ln = _build('nature_bf16', 0.0, spread=False)
    assert ln._defer_fc and ln._defer_wgrad and not ln._det_wgrad and ln._clip == 0.0
    ln.step()
    assert ln.grad_norm is None and not hasattr(net, '_clip_stats')


@pytest.mark.parametrize('flags', ['--dtype=bf16', '--dtype=fp16 ' + RAINBOW])
def test_flag_on_adds_exactly_the_clip_launches_to_the_unfused_step(monkeypatch, flags):
    """Against the same step with --fuse_fc_wgrad 0 --fuse_wgrad_update 0: one grad_clip call (its two
    launches) per step before the optimizer launch, and for noisy nets the explicit sigma-gradient
    launch and the noise draw the fused optimizer otherwise absorbs; nothing else differs."""
    monkeypatch.setitem(lt.CONFIGS, 'clip_on', ('nature', flags + ' --max_grad_norm=10', {}))
    monkeypatch.setitem(lt.CONFIGS, 'unfused', ('nature', flags + ' --fuse_fc_wgrad=0 --fuse_wgrad_update=0', {}))
    on, off = _names(lt.record_steps('clip_on')), _names(lt.record_steps('unfused'))
    # (grad_clip_blocks is the host-side size query of the first step: it launches nothing)
    assert on.count('grad_clip_blocks') == 1, on
    on = [n for n in on if n != 'grad_clip_blocks']
    assert on.count('grad_clip') == 2, on                       # two steps recorded
    i = on.index('grad_clip')
    assert on[i + 1] == 'optim_pack' or (on[i + 1] == 'noise_normal' and on[i + 2] == 'optim_pack'), on
    rest = [n for n in on if n != 'grad_clip']
    if 'noisy' not in flags:
        assert rest == off, (rest, off)
    else:
        extra = [n for n in rest if n in ('qnet_noisy_grad', 'noise_normal')]
        assert [n for n in rest if n not in ('qnet_noisy_grad', 'noise_normal')] == \
            [n for n in off if n not in ('qnet_noisy_grad', 'noise_normal')], (rest, off)
        assert extra.count('qnet_noisy_grad') == 2, rest
