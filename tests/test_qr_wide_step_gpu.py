"""The shipped SGD step of a QR-DQN net with more than 64 quantiles per action (nature + --quantile
--num_quantiles=200 --dueling --double_dqn: the paper's QR-DQN-1 count) on the HIP executor: the
wide QR head (csrc/kernels/qr_wide_head.hip) between the output-layer igemm over KD = 6 * 200 +
pad + 224 columns and the dH igemm / grouped weight gradients, as one HIP graph per step.

The method, thresholds and helpers are those of test_qr_step_gpu.py: every tensor's gradient is
recovered from the update and compared with ``TorchExecutor(oracle=True)`` (cosine > 0.985 and
norm within 5 % on the 16-bit builds, cosine > 0.9999 and norm within 0.2 % on fp32), the loss
and Q values against the oracle, and graph replay == the eager step. Before this head existed the
configuration fell back to the torch executor, which ``ex.name == 'hip'`` shows.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
QR200 = '--quantile --num_quantiles=200 --dueling --double_dqn'
RAINBOW_QR68 = '--quantile --num_quantiles=68 --dueling --double_dqn --noisy --prioritized_replay --optimizer=adam'
CAP = 65536            # large replay: the actors' 4 appends per step never touch the sampled rows


def _build(extra, acting, dtype, atoms, cap=CAP, lr=0.01, use_graph=True, seed=0, spread=False):
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    cfg = preset('nature', 'Pong-v0', '--seed=%d --backend=hip --dtype=%s --replay_memory_capacity=%d --lr=%g %s'
                 % (seed, dtype, cap, lr, extra))
    net = Network.create_network(cfg, (84, 84, 4), 6, device=DEV)
    ex = net.executor
    assert ex.name == 'hip' and ex.dist and ex.quantile and ex.atoms == atoms == cfg.num_quantiles == net.arch.atoms
    if spread:                                 # every layer carries signal
        g = torch.Generator(device=DEV).manual_seed(7)
        net.online.flat.normal_(0.0, 0.03, generator=g)
        net.target.flat.normal_(0.0, 0.03, generator=g)
        net.refresh_packed()
    rep = DeviceReplay(cap, (84, 84), 4, device=DEV, prioritized=cfg.prioritized_replay, seed=3)
    rep.fill_synthetic(cap, 6, seed=3)
    actor = None
    if acting:
        from dist_dqn_amd.actors.device_actor import DeviceActor
        actor = DeviceActor(net, rep, cfg, num_envs=4, steps_per_call=1, seed=11)
        assert actor.can_fuse(cfg.minibatch_size)
    return cfg, net, rep, Learner(net, rep, cfg, use_graph=use_graph, actor=actor)


@pytest.mark.parametrize('extra,atoms,acting,dtype', [(QR200, 200, False, 'bf16'), (QR200, 200, True, 'bf16'),
                                                      (QR200, 200, True, 'fp32'), (RAINBOW_QR68, 68, True, 'fp16')])
def test_qr_wide_production_step_matches_fp32_oracle_every_tensor(extra, atoms, acting, dtype):
    from dist_dqn_amd.models.executor import TorchExecutor
    cfg, net, rep, ln = _build(extra, acting, dtype, atoms, lr=0.0001 if 'adam' in extra else 0.01, spread=True)
    for _ in range(4):                         # eager warm-up, graph capture, then graph replays
        ln.step()
    torch.cuda.synchronize()
    assert ln._graphs is not None, 'the production step runs as a HIP graph'
    assert ln._sample_mode() == 'opt' and ln._presampled, 'next minibatch drawn by the optimizer launch'
    assert (ln.actor is not None) == acting
    sb = rep.slot_batch(cfg.minibatch_size)
    idx = sb['idx'].clone()
    batch = {k: v.clone() for k, v in rep.gather(idx).items()}
    if 'weights' in sb:
        batch['weights'] = sb['weights'].clone()
    w0, tgt0 = net.online.flat.clone(), net.target.flat.clone()
    s0 = [s.clone() for s in net.optimizer.slots]
    noise = net.noise.clone() if getattr(net, 'noise', None) is not None else None
    tnoise = net.noise_target.clone() if getattr(net, 'noise_target', None) is not None else None
    oracle = TorchExecutor(net.arch, net.layout, input_scale=cfg.input_scale, loss=cfg.loss, oracle=True,
                           huber_delta=cfg.huber_delta, double_dqn=cfg.double_dqn)
    # Q = mean of the quantiles, from the wide inference kernel
    q, q_ref = net.q_values(batch['states']), oracle.q_values(w0, batch['states'], noise)
    rel = float((q - q_ref).norm() / (q_ref.norm() + 1e-12))
    print('q_values rel err %.3g' % rel)
    assert q.shape == (cfg.minibatch_size, 6) and rel < (1e-4 if dtype == 'fp32' else 2e-2)
    frames0 = ln.actor.env_frames if acting else 0
    loss = ln.step()
    torch.cuda.synchronize()
    assert not torch.equal(net.online.flat, w0)
    assert not acting or ln.actor.env_frames == frames0 + 4
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
    loss_ref, _ = oracle.loss_and_grad(w0, tgt0, batch, g_ref, noise, tnoise)
    torch.cuda.synchronize()
    print('loss %.6g (oracle %.6g)' % (float(loss), float(loss_ref)))
    assert abs(float(loss) - float(loss_ref)) <= (1e-4 if dtype == 'fp32' else 3e-2) * abs(float(loss_ref))
    tol = (0.9999, 2e-3) if dtype == 'fp32' else (0.985, 0.05)
    checked, worst = [], (2.0, 0.0)
    for name in lay.names:
        o, k = lay.offsets[name], lay.numel(name)
        a, b = g_rec[o:o + k].double(), g_ref[o:o + k].double()
        if float(b.norm()) == 0.0:
            continue
        cos = float(torch.nn.functional.cosine_similarity(a, b, dim=0))
        ratio = float(a.norm() / b.norm())
        worst = (min(worst[0], cos), max(worst[1], abs(ratio - 1.0)))
        assert cos > tol[0] and abs(ratio - 1.0) < tol[1], (extra, acting, dtype, name, cos, ratio)
        checked.append(name)
    print('worst cosine %.6f, worst |norm ratio - 1| %.3g over %d tensors' % (worst + (len(checked),)))
    assert len(checked) >= 12, checked
    assert any(n.startswith('conv1') for n in checked) and any('value/output' in n for n in checked)
    assert any('advantage/output' in n for n in checked) and any('fcl' in n for n in checked)


def test_qr_wide_step_graph_equals_eager():
    """HIP-graph replay of the 200-quantile step == the same step run eagerly (parameters after the same steps)."""
    outs = []
    for graph in (False, True):
        _, net, _, ln = _build(QR200, False, 'bf16', 200, cap=4096, use_graph=graph, seed=3)
        for _ in range(4):                     # (graph: eager warm-up, capture, then one replayed step)
            ln.step()
        torch.cuda.synchronize()
        assert int(net.global_step) == 4 and (ln._graphs is not None) == graph
        outs.append(net.online.flat.clone())
    # wgrad combines M-chunks with fp32 atomics (order-dependent last bits)
    torch.testing.assert_close(outs[0], outs[1], rtol=1e-4, atol=1e-6)
