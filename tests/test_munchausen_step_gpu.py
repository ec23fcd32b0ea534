"""The shipped SGD step of a Munchausen-DQN net (nature + --munchausen --dueling --loss=huber) on
the HIP executor: one HIP graph per step, three learner instances (online(s), target(s'),
target(s)), the Munchausen head (csrc/kernels/mdqn_head.hip) between the rows path's output-layer
igemm and its dH igemm / grouped weight gradients, the fused optimizer launch that also draws the
next minibatch, and (``acting``) the device actors' step in the head launch's acting blocks.

* every tensor's gradient against ``TorchExecutor(oracle=True)``, recovered from the update as
  test_production_step_gpu.py does (RMSProp: g = (w - w') sqrt(ms' + eps) / lr; Adam:
  g = (m' - b1 m) / (1 - b1); minus the L2 term), to test_qr_step_gpu.py's thresholds: cosine >
  0.985 and norm within 5 % on the 16-bit builds, cosine > 0.9999 and norm within 0.2 % on fp32;
* the loss and the Q values against the oracle, to that file's bounds;
* graph replay == the eager step, and ``step_many(4)`` == four single steps, to that file's
  tolerance;
* the same on a noisy, prioritized Adam net in fp16 and on the reference `cnn` in bf16.

The reference `cnn` case runs at lr 1e-3, not the 0.01 of the nature cases: TF RMSProp's first
steps move a weight by about 2-4 lr each, so the four warm-up steps at 0.01 displace every weight
by more than the 0.03 spread of the initialisation and the step under test no longer sees the
spread net (a plain cnn net ends at |Q| up to 70, a Munchausen one collapsed to |Q| < 1), while
at 1e-3 they stay a fraction of it. The cnn preset feeds raw uint8 pixels (input_scale 1), and
the absolute error of a bf16 Q value follows the activations' scale, not |Q|: measured 0.03-0.07
per |td| in every one of these regimes. Figures of the one MI355X run, bf16, same thresholds:
lr 1e-3: Q rel err 0.011, loss 0.3229 (oracle 0.3175), worst cosine 0.9957, worst norm ratio
0.970 (passes); lr 0.01: Q 0.003, loss within 1.8 %, but conv2/w cosine 0.930 and conv3/w 0.975
(|td| about 0.4, so that error is 10 % of every dL/dQ of the MSE loss; the fp32 build of the same
step agrees with the oracle to 6e-6 in every |td|, and bf16 with alpha = 0 or tau = 1, |td| of
2-10, reaches cosine 0.9999); lr 1e-4: cosines >= 0.990 but Q rel err 0.0216 against the 0.02
bound (a plain cnn net there: 0.0163).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
MD = '--munchausen --dueling --loss=huber'
NOISY_MD = '--munchausen --noisy --prioritized_replay --optimizer=adam'
CAP = 65536            # large replay: the actors' 4 appends per step never touch the sampled rows


def _build(extra, acting, dtype, cap=CAP, lr=0.01, use_graph=True, seed=0, spread=False, env_type='nature'):
    from dist_dqn_amd.config import preset
    from dist_dqn_amd.learner import Learner
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import DeviceReplay
    cfg = preset(env_type, 'Pong-v0', '--seed=%d --backend=hip --dtype=%s --replay_memory_capacity=%d --lr=%g %s'
                 % (seed, dtype, cap, lr, extra))
    net = Network.create_network(cfg, (84, 84, 4), 6, device=DEV)
    ex = net.executor
    assert ex.name == 'hip' and ex.mdqn == (cfg.m_alpha, cfg.m_tau, cfg.m_clip) and ex.rows
    assert not ex.dist and ex.atoms == 1 and not net.arch.distributional and not ex.can_fold_head(cfg.minibatch_size)
    assert type(ex).__name__ == ('HipCnnExecutor' if env_type == 'atari' else 'HipExecutor')
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


@pytest.mark.parametrize('extra,acting,dtype,env_type', [
    (MD, False, 'bf16', 'nature'), (MD, True, 'bf16', 'nature'), (MD, False, 'fp32', 'nature'),
    (MD, True, 'fp32', 'nature'), (NOISY_MD, True, 'fp16', 'nature'), ('--munchausen', False, 'bf16', 'atari')])
def test_munchausen_production_step_matches_fp32_oracle_every_tensor(extra, acting, dtype, env_type):
    from dist_dqn_amd.models.executor import TorchExecutor
    # (the reference `cnn` runs at lr 1e-3: see the module docstring)
    lr = 0.0001 if 'adam' in extra else 0.001 if env_type == 'atari' else 0.01
    cfg, net, rep, ln = _build(extra, acting, dtype, lr=lr, spread=True, env_type=env_type)
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
                           huber_delta=cfg.huber_delta, munchausen=(cfg.m_alpha, cfg.m_tau, cfg.m_clip))
    # plain Q from the inference kernel (acting is eps-greedy on Q)
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
    assert len(checked) >= (12 if '--dueling' in extra else 10), checked
    assert any(n.startswith('conv1') for n in checked) and any('fcl' in n for n in checked)
    if '--dueling' in extra:
        assert any('value/output' in n for n in checked) and any('advantage/output' in n for n in checked)
    else:
        assert any(n.startswith('output') for n in checked)


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_munchausen_step_graph_equals_eager(dtype):
    """HIP-graph replay of the step == the same step run eagerly (parameters after the same steps)."""
    outs = []
    for graph in (False, True):
        _, net, _, ln = _build(MD, False, dtype, cap=4096, use_graph=graph, seed=3)
        for _ in range(4):                     # (graph: eager warm-up, capture, then one replayed step)
            ln.step()
        torch.cuda.synchronize()
        assert int(net.global_step) == 4 and (ln._graphs is not None) == graph
        outs.append(net.online.flat.clone())
    # wgrad combines M-chunks with fp32 atomics (order-dependent last bits)
    torch.testing.assert_close(outs[0], outs[1], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('extra,mode', [('--target_update_tau=0.01', 'launch'), ('--fuse_sampling=0', 'launch'),
                                        ('--target_update_tau=0.01 --prioritized_replay', 'launch')])
def test_munchausen_step_without_the_optimizer_drawn_minibatch(extra, mode):
    """Polyak target updates (no fused hard sync, so the optimizer launch draws no minibatch) and
    --fuse_sampling=0: the learner must fall to the sampler launch, never to the trunk's in-kernel
    sampling (which reads next-state slots for the third instance); the step runs as a graph, the
    target moves every step under Polyak, and the step's gradient matches the oracle's."""
    from dist_dqn_amd.models.executor import TorchExecutor
    cfg, net, rep, ln = _build(MD + ' ' + extra, False, 'bf16', spread=True)
    assert net.executor.name == 'hip' and not net.executor.fused_sampling
    assert ln._sample_mode() == mode
    for _ in range(4):
        ln.step()
    torch.cuda.synchronize()
    assert ln._graphs is not None and int(net.global_step) == 4
    tgt0, w0 = net.target.flat.clone(), net.online.flat.clone()
    loss = ln.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and not torch.equal(net.online.flat, w0)
    if 'tau' in extra:
        assert not torch.equal(net.target.flat, tgt0) and not torch.equal(net.target.flat, net.online.flat)
    # the eager step on a fixed batch against the oracle (loss and every tensor's gradient)
    beta = (net.global_step, cfg.per_beta0, cfg.per_beta_steps) if cfg.prioritized_replay else None
    batch = rep.sample_slots(cfg.minibatch_size, beta)
    assert 'sample_spec' not in batch
    full = {k: v.clone() for k, v in rep.gather(batch['idx']).items()}
    if 'weights' in batch:
        full['weights'] = batch['weights'].clone()
    g_hip, g_ref = torch.zeros_like(w0), torch.zeros_like(w0)
    w1, t1 = net.online.flat.clone(), net.target.flat.clone()
    loss_h, prio_h = net.executor.loss_and_grad(net.online.flat, net.target.flat, batch, g_hip)
    oracle = TorchExecutor(net.arch, net.layout, input_scale=cfg.input_scale, loss=cfg.loss, oracle=True,
                           huber_delta=cfg.huber_delta, munchausen=(cfg.m_alpha, cfg.m_tau, cfg.m_clip))
    loss_r, _ = oracle.loss_and_grad(w1, t1, full, g_ref)
    torch.cuda.synchronize()
    assert abs(float(loss_h) - float(loss_r)) <= 3e-2 * abs(float(loss_r)), (float(loss_h), float(loss_r))
    lay = net.layout
    for name in lay.names:
        o, k = lay.offsets[name], lay.numel(name)
        a, b = g_hip[o:o + k].double(), g_ref[o:o + k].double()
        if float(b.norm()) == 0.0:
            continue
        cos = float(torch.nn.functional.cosine_similarity(a, b, dim=0))
        assert cos > 0.985 and abs(float(a.norm() / b.norm()) - 1.0) < 0.05, (name, cos)


def test_munchausen_step_many_equals_single_steps():
    """Learner.step_many(4) (ONE graph holding four step bodies) == four separate step() replays."""
    outs = []
    for many in (False, True):
        _, net, _, ln = _build(MD + ' --target_update_freq=5', False, 'bf16', cap=4096, seed=3)
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
        outs.append((net.online.flat.clone(), net.target.flat.clone()))
    # (conv weight gradients combine M-chunks with fp32 atomics: order-dependent last bits)
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-6)
