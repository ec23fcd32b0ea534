"""Munchausen-DQN on the CPU: the torch loss (models/losses.py munchausen_loss) against an
independent float64 transcription of its formulas, the target's identities, the --munchausen
flags and refusals, the parameter layout, a TorchExecutor step and a short CartPole run.

Target (Vieillard, Pietquin, Geist 2020), q' = target net on s', q0 = target net on s:
  soft = max q' + tau log sum_k exp((q'_k - max q') / tau)
  lp   = q0_a - max q0 - tau log sum_k exp((q0_k - max q0) / tau)            (<= 0)
  y    = r + alpha clip(lp, l0, 0) + gamma (1 - done) soft,   d = Q(s, a) - y
per-sample loss d^2 (MSE) or Huber_delta(d), priority |d|, loss = mean_b w_b per_b;
d loss / d Q(s, a) = w_b / B * (2 d or clamp(d, -delta, delta)), zero for the other actions.

Rows of every batch: 1 and 4 are terminal, 2 has gamma = 0, every input of row 3 is scaled by
1e3 (with tau = 0.03 the exponents reach -1e5: the max-subtracted form stays finite where
exp(q / tau) would overflow); gammas are 0.99^{1, 2, 3}; the 'zero' weights hold an exact 0 on row 5.

Bounds: the torch function computes in fp32, the reference in float64 on the same fp32 inputs.
d is a sum of a handful of fp32 terms (each rounded at the size of the row's Q values), so the
priority, the loss and the gradient are compared with rtol 1e-5 and an atol of 1e-5 times the
row's largest |Q| (the 1e-5 relative bound of the issue for the scaled row, where |d| ~ |Q|).
"""
import numpy as np
import pytest
import torch

B = 12


def _case(A, tau, wmode, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, A, generator=g)
    qn = torch.randn(B, A, generator=g)
    qs = torch.randn(B, A, generator=g)
    act = torch.randint(0, A, (B,), generator=g)
    rew = torch.randn(B, generator=g)
    done = torch.zeros(B)
    done[1] = done[4] = 1.0
    gam = torch.tensor([0.99 ** (1 + i % 3) for i in range(B)])
    gam[2] = 0.0
    for t in (q, qn, qs):
        t[3] *= 1e3
    rew[3] *= 1e3
    wts = None
    if wmode != 'none':
        wts = torch.rand(B, generator=g) + 0.5
        if wmode == 'zero':
            wts[5] = 0.0
    return dict(A=A, tau=tau, q=q, qn=qn, qs=qs, act=act, rew=rew, done=done, gam=gam, wts=wts)


def _soft64(x, tau):
    m = x.max(-1)
    return m + tau * np.log(np.exp((x - m[..., None]) / tau).sum(-1)), m


def _reference(c, alpha, clip, kind, delta):
    """(loss, |d| [B], grad [B, A], bonus [B], soft [B]) in float64."""
    tau = float(c['tau'])
    q, qn, qs = (c[n].double().numpy() for n in ('q', 'qn', 'qs'))
    rew, done, gam = (c[n].double().numpy() for n in ('rew', 'done', 'gam'))
    w = np.ones(B) if c['wts'] is None else c['wts'].double().numpy()
    act = c['act'].numpy()
    rows = np.arange(B)
    soft, _ = _soft64(qn, tau)
    lse0, m0 = _soft64(qs, tau)
    lp = qs[rows, act] - m0 - (lse0 - m0)
    bonus = alpha * np.clip(lp, clip, 0.0)
    y = rew + bonus + gam * (1.0 - done) * soft
    d = q[rows, act] - y
    if kind == 'mse':
        per, g = d * d, 2.0 * d
    else:
        ad = np.abs(d)
        per = np.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta))
        g = np.clip(d, -delta, delta)
    grad = np.zeros((B, c['A']))
    grad[rows, act] = w / B * g
    return float((w * per).sum() / B), np.abs(d), grad, bonus, soft


CASES = [(A, tau, kind, delta, wmode) for A in (2, 6, 18) for tau in (0.03, 1.0)
         for kind, delta, wmode in (('mse', 1.0, 'none'), ('huber', 1.0, 'rand'), ('huber', 0.5, 'zero'),
                                    ('mse', 1.0, 'zero'))]


@pytest.mark.parametrize('A,tau,kind,delta,wmode', CASES)
def test_munchausen_loss_value_and_gradient(A, tau, kind, delta, wmode):
    from dist_dqn_amd.models.losses import munchausen_loss
    c = _case(A, tau, wmode, 100 * A + int(10 * tau))
    alpha, clip = 0.9, -1.0
    loss_ref, ad_ref, grad_ref, bonus, _ = _reference(c, alpha, clip, kind, delta)
    q = c['q'].clone().requires_grad_(True)
    loss, prio = munchausen_loss(q, c['act'], c['rew'], c['done'], c['qn'], c['qs'], c['gam'], alpha, tau, clip,
                                 kind, delta, c['wts'])
    loss.backward()
    assert prio.shape == (B,) and not prio.requires_grad
    assert torch.isfinite(prio).all() and torch.isfinite(loss) and torch.isfinite(q.grad).all()
    mag = np.maximum(1.0, np.abs(np.stack([c[n].double().numpy() for n in ('q', 'qn', 'qs')])).max((0, 2)))
    assert mag[3] > 500.0                                           # the scaled row
    err = np.abs(prio.double().numpy() - ad_ref)
    assert (err <= 1e-5 * ad_ref + 1e-5 * mag).all(), (err, ad_ref)
    # the scaled row against float64 to 1e-5 relative (|d| there is of the size of its Q values)
    assert ad_ref[3] > 100.0 and err[3] <= 1e-5 * max(ad_ref[3], mag[3])
    gerr = np.abs(q.grad.double().numpy() - grad_ref)
    gscale = (2.0 if kind == 'mse' else 0.0) * mag[:, None] / B      # d(grad) / d(d) = 2 w / B (MSE), clipped: 0
    assert (gerr <= 1e-5 * np.abs(grad_ref) + 1e-5 * gscale * 1.5 + 1e-7).all(), gerr.max()
    big = kind == 'mse'                                              # the scaled row's d^2 dominates the MSE loss
    np.testing.assert_allclose(float(loss.detach()), loss_ref, rtol=3e-5 if big else 1e-5, atol=1e-5)
    assert (bonus <= 0).all() and (bonus >= alpha * clip).all()
    if wmode == 'zero':
        assert float(q.grad[5].abs().max()) == 0.0 and float(prio[5]) > 0.0
    # terminal rows and gamma = 0 rows see no next-state value
    c2 = dict(c, qn=c['qn'] + 7.0)
    _, prio2 = munchausen_loss(c['q'], c['act'], c['rew'], c['done'], c2['qn'], c['qs'], c['gam'], alpha, tau, clip,
                               kind, delta, c['wts'])
    for b in (1, 2, 4):
        assert float(prio2[b]) == float(prio[b])
    assert float(prio2[0]) != float(prio[0])


def test_munchausen_loss_takes_scalar_and_column_gamma():
    from dist_dqn_amd.models.losses import munchausen_loss
    c = _case(4, 0.03, 'rand', 5)
    args = (c['q'], c['act'], c['rew'], c['done'], c['qn'], c['qs'])
    a = munchausen_loss(*args, c['gam'], weights=c['wts'])
    b = munchausen_loss(*args, c['gam'].view(-1, 1), weights=c['wts'])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c['gam'][:] = 0.9
    a = munchausen_loss(*args, c['gam'], weights=c['wts'])
    b = munchausen_loss(*args, 0.9, weights=c['wts'])
    torch.testing.assert_close(a[1], b[1], rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------ identities of the target
@pytest.mark.parametrize('A', [2, 6, 18])
@pytest.mark.parametrize('tau', [0.03, 1.0])
def test_soft_value_lies_between_max_and_max_plus_tau_log_a(A, tau):
    """max q <= soft <= max q + tau log A, read off the loss with alpha = 0, r = 0, gamma = 1, Q(s, a) = 0."""
    from dist_dqn_amd.models.losses import munchausen_loss
    c = _case(A, tau, 'none', 7 * A)
    z = torch.zeros(B)
    _, prio = munchausen_loss(torch.zeros(B, A), c['act'], z, z, c['qn'], c['qs'], 1.0, 0.0, tau, -1.0)
    _, _, _, _, soft64 = _reference(c, 0.0, -1.0, 'mse', 1.0)
    qn = c['qn'].double().numpy()
    mx = qn.max(1)
    tol = 4e-7 * np.maximum(1.0, np.abs(mx))                         # fp32 rounding of soft itself
    soft = np.where(soft64 >= 0, 1.0, -1.0) * prio.double().numpy()  # |0 - soft| with float64's sign
    assert (soft >= mx - tol).all() and (soft <= mx + tau * np.log(A) + tol).all()
    assert (soft64 >= mx).all() and (soft64 <= mx + tau * np.log(A) + 1e-12).all()


def test_alpha_zero_small_tau_is_the_plain_dqn_target():
    """alpha = 0, tau = 1e-4: y = r + gamma (1 - done) max q' within gamma tau log A."""
    from dist_dqn_amd.models.losses import munchausen_loss, scalar_td_loss
    A, tau = 6, 1e-4
    c = _case(A, tau, 'none', 11)
    for t in ('q', 'qn', 'qs'):
        c[t][3] /= 1e3                                              # (keep fp32 rounding below tau log A)
    c['rew'][3] /= 1e3
    _, pm = munchausen_loss(c['q'], c['act'], c['rew'], c['done'], c['qn'], c['qs'], c['gam'], 0.0, tau, -1.0)
    _, pd = scalar_td_loss(c['q'], c['act'], c['rew'], c['done'], c['qn'], None, c['gam'])
    assert (pm - pd).abs().max() <= tau * np.log(A) + 1e-6


@pytest.mark.parametrize('alpha,clip', [(0.9, -1.0), (1.0, -0.25), (0.0, -1.0)])
def test_bonus_lies_in_alpha_l0_to_zero(alpha, clip):
    """y(alpha) - y(0) = alpha clip(lp, l0, 0) in [alpha l0, 0], read off two losses."""
    from dist_dqn_amd.models.losses import munchausen_loss
    c = _case(6, 0.03, 'none', 13)
    for t in ('q', 'qn', 'qs'):
        c[t][3] /= 1e3
    c['rew'][3] /= 1e3
    q = torch.full((B, 6), 1e3)                                      # d = Q - y > 0 everywhere: |d| = d
    args = (q, c['act'], c['rew'], c['done'], c['qn'], c['qs'], c['gam'])
    _, p1 = munchausen_loss(*args, alpha, 0.03, clip)
    _, p0 = munchausen_loss(*args, 0.0, 0.03, clip)
    bonus = (p0 - p1).double().numpy()                               # (Q - y0) - (Q - y1) = y1 - y0
    assert (bonus <= 2e-4).all() and (bonus >= alpha * clip - 2e-4).all()     # fp32 at |Q| = 1e3
    _, _, _, ref, _ = _reference(c, alpha, clip, 'mse', 1.0)
    assert (ref <= 0).all() and (ref >= alpha * clip).all()
    np.testing.assert_allclose(bonus, ref, atol=2e-4)
    if alpha > 0:
        assert (ref == alpha * clip).any() and (ref > alpha * clip).any()      # both sides of the clip occur


# ------------------------------------------------------------------ flags, config, layout
def test_munchausen_flag_defaults_and_config_fields():
    from dist_dqn_amd.config import Config, defaults, flag_names, parse_args
    d = defaults()
    for c in (d, Config()):
        assert c.munchausen is False and c.m_alpha == 0.9 and c.m_tau == 0.03 and c.m_clip == -1.0
    assert {'munchausen', 'm_alpha', 'm_tau', 'm_clip'} <= set(flag_names())
    c = parse_args(['--munchausen', '--m_alpha=0.5', '--m_tau=1', '--m_clip=-2', '--dueling', '--loss=huber'])
    assert c.munchausen is True and c.m_alpha == 0.5 and c.m_tau == 1.0 and c.m_clip == -2.0
    assert c.distributional is False and c.double_dqn is False
    assert parse_args(['--munchausen', '--m_alpha=0']).m_alpha == 0.0
    assert parse_args(['--munchausen', '--m_alpha=1', '--fuse_sampling=0']).fuse_sampling == 0
    assert parse_args(['--munchausen']).fuse_sampling == 2
    # without the flag nothing is checked or changed
    assert parse_args(['--double_dqn', '--fuse_sampling=1', '--m_tau=0']).munchausen is False


@pytest.mark.parametrize('argv,words', [
    (['--munchausen', '--distributional'], ('--munchausen and --distributional cannot be combined',)),
    (['--munchausen', '--quantile'], ('--munchausen and --quantile cannot be combined',)),
    (['--munchausen', '--double_dqn'], ('--munchausen and --double_dqn cannot be combined', 'argmax')),
    (['--munchausen', '--fuse_sampling=1'], ('--munchausen and --fuse_sampling=1 cannot be combined',)),
    (['--munchausen', '--m_alpha=1.5'], ('--m_alpha', '[0, 1]')),
    (['--munchausen', '--m_alpha=-0.1'], ('--m_alpha', '[0, 1]')),
    (['--munchausen', '--m_tau=0'], ('--m_tau', '> 0')),
    (['--munchausen', '--m_clip=0'], ('--m_clip', '< 0')),
    (['--munchausen', '--m_clip=0.5'], ('--m_clip', '< 0'))])
def test_munchausen_flag_refusals(argv, words, capsys):
    from dist_dqn_amd.config import parse_args
    with pytest.raises(SystemExit):
        parse_args(argv)
    err = capsys.readouterr().err
    for w in words:
        assert w in err, (w, err)


@pytest.mark.parametrize('network,shape', [('nature', (84, 84, 4)), ('cnn', (84, 84, 4)), ('simple', (4,))])
@pytest.mark.parametrize('extra', [[], ['--dueling'], ['--dueling', '--noisy']])
def test_munchausen_keeps_the_plain_arch_and_layout(network, shape, extra):
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.models.arch import arch_from_config
    from dist_dqn_amd.models.params import FlatLayout
    base = ['--network=%s' % network] + extra
    m = arch_from_config(parse_args(base + ['--munchausen']), shape, 6)
    p = arch_from_config(parse_args(base), shape, 6)
    assert m == p and not m.distributional and m.atoms == 1 and m.param_specs() == p.param_specs()
    lm, lp = FlatLayout(m), FlatLayout(p)
    assert lm.names == lp.names and lm.offsets == lp.offsets and lm.total == lp.total


def test_executor_choice():
    """`simple` + --munchausen is declined by the MLP executor; conv nets up to 32 actions are
    taken by the HIP executor, larger action sets are not."""
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.models.arch import arch_from_config
    from dist_dqn_amd.models.executor import TorchExecutor, check_munchausen
    from dist_dqn_amd.ops.executor import supports
    from dist_dqn_amd.ops.mlp_executor import supports_mlp
    s = arch_from_config(parse_args(['--network=simple', '--munchausen']), (4,), 2)
    assert supports_mlp(s) and not supports_mlp(s, (0.9, 0.03, -1.0))
    hp = (0.9, 0.03, -1.0)
    for net in ('nature', 'cnn'):
        a32 = arch_from_config(parse_args(['--network=%s' % net, '--munchausen', '--dueling']), (84, 84, 4), 32)
        a33 = arch_from_config(parse_args(['--network=%s' % net, '--munchausen']), (84, 84, 4), 33)
        assert supports(a32, hp) and supports(a33) and not supports(a33, hp)
    c51 = arch_from_config(parse_args(['--network=nature', '--distributional']), (84, 84, 4), 6)
    assert supports(c51) and not supports(c51, hp)
    from dist_dqn_amd.models.params import FlatLayout
    with pytest.raises(RuntimeError, match='double_dqn'):
        TorchExecutor(s, FlatLayout(s), double_dqn=True, munchausen=hp)
    with pytest.raises(RuntimeError, match='munchausen'):
        TorchExecutor(c51, FlatLayout(c51), munchausen=hp)
    for bad in ((1.5, 0.03, -1.0), (0.9, 0.0, -1.0), (0.9, 0.03, 0.0)):
        with pytest.raises(RuntimeError, match='m_tau'):
            check_munchausen(s, False, *bad)


# ------------------------------------------------------------------ a step and a short run on the CPU
def test_torch_executor_step_on_simple():
    """One TorchExecutor step of a CartPole-sized dueling net: finite loss, a nonzero gradient,
    and the loss of munchausen_loss on the three forwards."""
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.models import torch_net
    from dist_dqn_amd.models.losses import munchausen_loss
    from dist_dqn_amd.models.network import Network
    cfg = parse_args(['--device=cpu', '--seed=1', '--network=simple', '--munchausen', '--dueling', '--loss=huber',
                      '--optimizer=adam', '--lr=0.01', '--reg_param=0'])
    net = Network.create_network(cfg, (4,), 2)
    ex = net.executor
    assert ex.name == 'torch' and ex.munchausen == (0.9, 0.03, -1.0) and not net.arch.distributional
    g = torch.Generator().manual_seed(3)
    n = 16
    batch = {'states': torch.randn(n, 4, generator=g), 'next_states': torch.randn(n, 4, generator=g),
             'actions': torch.randint(0, 2, (n,), generator=g), 'rewards': torch.randn(n, generator=g),
             'dones': (torch.rand(n, generator=g) < 0.3).float(), 'gammas': torch.full((n,), 0.9)}
    fwd = lambda flat, x: torch_net.forward(net.arch, flat, net.layout, x)
    want, wprio = munchausen_loss(fwd(net.online.flat, batch['states']), batch['actions'], batch['rewards'],
                                  batch['dones'], fwd(net.target.flat, batch['next_states']),
                                  fwd(net.target.flat, batch['states']), batch['gammas'], 0.9, 0.03, -1.0, 'huber', 1.0)
    loss, prio = net.compute_grads(batch)
    assert torch.isfinite(loss).all() and torch.isfinite(net.grad).all() and float(net.grad.abs().max()) > 0.0
    torch.testing.assert_close(loss.view(()), want)
    torch.testing.assert_close(prio, wprio)
    losses = []
    for _ in range(8):
        loss, prio = net.train_step(batch)
        assert prio.shape == (n,) and torch.isfinite(prio).all() and (prio >= 0).all()
        losses.append(float(loss))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_cartpole_agent_runs_with_munchausen(tmp_path):
    """A short DQNAgent.train run on the CPU (wiring, not a learning claim), with n-step returns
    and reward clipping on: the bonus is that of the sampled (s, a), the reward is stored clipped."""
    from dist_dqn_amd.agent import DQNAgent
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.envs import CartPoleEnv
    from dist_dqn_amd.models.network import Network
    from dist_dqn_amd.replay import ReplayMemory
    cfg = parse_args(['--device=cpu', '--seed=0', '--logdir=%s' % tmp_path, '--network=simple', '--munchausen',
                      '--loss=huber', '--optimizer=adam', '--lr=0.002', '--minibatch_size=16', '--n_step=3',
                      '--reward_clip=1', '--replay_start_size=32', '--target_update_freq=20', '--reg_param=0',
                      '--max_train_steps=60'])
    env = CartPoleEnv(seed=0)
    net = Network.create_network(cfg, (4,), 2)
    assert net.executor.name == 'torch' and net.executor.munchausen is not None
    before = net.online.flat.clone()
    agent = DQNAgent(env, net, None, ReplayMemory(2000), cfg, enable_summary=False)
    agent.train(20, 50)
    assert agent.training_steps >= 20 and int(net.global_step) == agent.training_steps
    assert torch.isfinite(net.online.flat).all() and not torch.equal(before, net.online.flat)
    assert np.isfinite(float(net.last_loss))
