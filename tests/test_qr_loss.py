"""QR-DQN on the CPU: the torch quantile regression loss (models/losses.py qr_loss) against an
independent float64 implementation with explicit loops, its autograd gradient against the closed
form, the --quantile flags, the architecture's widths, and a few TorchExecutor steps.

Loss (Dabney et al. 2018): tau_i = (2 i + 1) / 2 N, a* = first argmax_a of mean_j theta_sel(s', a)_j
(sel = online net on s' under Double DQN, else the target net), T_j = r + gamma (1 - done)
theta_target(s', a*)_j, u_ij = T_j - theta(s, a)_i,
rho_ij = |tau_i - 1{u_ij < 0}| L_kappa(u_ij) / kappa, per sample sum_i 1/N sum_j rho_ij (the PER
priority), loss = mean_b w_b per_b. Gradient: d loss / d theta(s, a)_i =
-(w_b / B) 1/N sum_j |tau_i - 1{u_ij < 0}| clamp(u_ij, -kappa, kappa) / kappa, zero for other actions.

Rows of every batch: 1 and 4 are terminal, 2 has |u| >= 40 kappa everywhere, 3 has T = theta
exactly (a constant row against a terminal reward of the same value: zero loss, zero gradient);
gammas are 0.99^{1, 2, 3}; the 'zero' weights hold an exact 0 on row 5.

Bounds: the torch function computes in fp32, the reference in float64 on the same fp32 inputs.
One rho term carries a few fp32 roundings of u (|u| eps) and the sums N^2 terms of one sign
pattern, so rtol 2e-5 with atol 1e-6 (values) / 1e-7 (gradient elements, which are <= w / B).
"""
import numpy as np
import pytest
import torch

B = 12


def _case(A, N, double, wmode, kappa, seed):
    g = torch.Generator().manual_seed(seed)
    th = torch.randn(B, A, N, generator=g)
    tt = torch.randn(B, A, N, generator=g)
    to = torch.randn(B, A, N, generator=g) if double else None
    act = torch.randint(0, A, (B,), generator=g)
    rew = torch.randn(B, generator=g)
    done = torch.zeros(B)
    done[1] = done[4] = 1.0
    gam = torch.tensor([0.99 ** (1 + i % 3) for i in range(B)])
    tt[2] = 50.0 + torch.randn(A, N, generator=g)                 # |u| far above kappa everywhere
    rew[2] = 100.0
    th[3, act[3]] = 0.75                                          # T = theta exactly
    rew[3], done[3] = 0.75, 1.0
    wts = None
    if wmode != 'none':
        wts = torch.rand(B, generator=g) + 0.5
        if wmode == 'zero':
            wts[5] = 0.0
    return dict(A=A, N=N, kappa=kappa, th=th, tt=tt, to=to, act=act, rew=rew, done=done, gam=gam, wts=wts)


def _reference(c):
    """(loss, per [B], grad [B, A, N], smallest gap between the two best selection means)."""
    A, N, k = c['A'], c['N'], float(c['kappa'])
    th, tt = c['th'].double().numpy(), c['tt'].double().numpy()
    sel = tt if c['to'] is None else c['to'].double().numpy()
    rew, done, gam = (c[n].double().numpy() for n in ('rew', 'done', 'gam'))
    w = np.ones(B) if c['wts'] is None else c['wts'].double().numpy()
    per, grad, gap = np.zeros(B), np.zeros((B, A, N)), np.inf
    for b in range(B):
        qs = [sum(sel[b, a, j] for j in range(N)) / N for a in range(A)]
        best = 0
        for a in range(1, A):
            if qs[a] > qs[best]:
                best = a
        top = sorted(qs)
        gap = min(gap, top[-1] - top[-2])
        a0 = int(c['act'][b])
        for i in range(N):
            tau = (2 * i + 1) / (2.0 * N)
            for j in range(N):
                u = rew[b] + gam[b] * (1.0 - done[b]) * tt[b, best, j] - th[b, a0, i]
                hub = 0.5 * u * u if abs(u) <= k else k * (abs(u) - 0.5 * k)
                wq = abs(tau - (1.0 if u < 0 else 0.0))
                per[b] += wq * hub / k / N
                grad[b, a0, i] -= w[b] / B * wq * min(max(u, -k), k) / k / N
    return float((w * per).sum() / B), per, grad, gap


CASES = [(A, N, double, wmode, kappa)
         for A in (2, 6) for N in (2, 21, 32, 64)
         for double, wmode, kappa in ((False, 'none', 1.0), (True, 'rand', 0.5), (True, 'zero', 1.0),
                                      (False, 'zero', 0.5))]


@pytest.mark.parametrize('A,N,double,wmode,kappa', CASES)
def test_qr_loss_value_and_gradient(A, N, double, wmode, kappa):
    from dist_dqn_amd.models.losses import qr_loss
    c = _case(A, N, double, wmode, kappa, 100 * A + N + int(double))
    loss_ref, per_ref, grad_ref, gap = _reference(c)
    assert gap > 1e-4, 'near-tie of the selection means in the reference: pick another seed'
    th = c['th'].clone().requires_grad_(True)
    loss, per = qr_loss(th, c['act'], c['rew'], c['done'], c['tt'], c['to'], c['gam'], kappa, c['wts'])
    loss.backward()
    assert per.shape == (B,) and not per.requires_grad
    np.testing.assert_allclose(per.double().numpy(), per_ref, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(float(loss.detach()), loss_ref, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(th.grad.double().numpy(), grad_ref, rtol=2e-5, atol=1e-7)
    assert per_ref[2] > 40.0 * kappa                               # the linear branch everywhere
    assert float(per[3]) == 0.0 and float(th.grad[3].abs().max()) == 0.0
    if wmode == 'zero':
        assert float(th.grad[5].abs().max()) == 0.0 and float(per[5]) > 0.0


def test_qr_loss_takes_scalar_and_column_gamma():
    from dist_dqn_amd.models.losses import qr_loss
    c = _case(3, 8, True, 'rand', 1.0, 5)
    a = qr_loss(c['th'], c['act'], c['rew'], c['done'], c['tt'], c['to'], c['gam'], 1.0, c['wts'])
    b = qr_loss(c['th'], c['act'], c['rew'], c['done'], c['tt'], c['to'], c['gam'].view(-1, 1), 1.0, c['wts'])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c['gam'][:] = 0.9
    a = qr_loss(c['th'], c['act'], c['rew'], c['done'], c['tt'], c['to'], c['gam'], 1.0, c['wts'])
    b = qr_loss(c['th'], c['act'], c['rew'], c['done'], c['tt'], c['to'], 0.9, 1.0, c['wts'])
    torch.testing.assert_close(a[1], b[1], rtol=1e-6, atol=1e-7)


def test_first_maximum_wins_on_an_exact_tie():
    from dist_dqn_amd.models.losses import qr_loss
    c = _case(4, 8, True, 'none', 1.0, 9)
    c['to'][0, 1] += 5.0
    c['to'][0, 3] = c['to'][0, 1]                                   # bit-identical greedy rows
    _, per_ref, _, _ = _reference(c)
    _, per = qr_loss(c['th'], c['act'], c['rew'], c['done'], c['tt'], c['to'], c['gam'], 1.0, None)
    np.testing.assert_allclose(per.double().numpy(), per_ref, rtol=2e-5, atol=1e-6)
    c['tt'][0, 3] += 100.0                                          # the later maximum's row is not used
    _, per2 = qr_loss(c['th'], c['act'], c['rew'], c['done'], c['tt'], c['to'], c['gam'], 1.0, None)
    assert torch.equal(per, per2)


# ------------------------------------------------------------------ flags and architecture
def test_quantile_flag_defaults():
    from dist_dqn_amd.config import Config, defaults, parse_args
    d = defaults()
    assert d.quantile is False and d.num_quantiles == 32 and d.qr_kappa == 1.0
    assert Config().quantile is False and Config().num_quantiles == 32 and Config().qr_kappa == 1.0
    c = parse_args(['--quantile', '--num_quantiles=51', '--qr_kappa=0.5'])
    assert c.quantile is True and c.num_quantiles == 51 and c.qr_kappa == 0.5 and c.distributional is False
    assert parse_args(['--quantile', '--num_quantiles=200']).num_quantiles == 200     # (torch executor)


@pytest.mark.parametrize('argv,word', [(['--quantile', '--distributional'], 'different distributional heads'),
                                       (['--quantile', '--num_quantiles=1'], 'must be at least 2'),
                                       (['--quantile', '--num_quantiles=0'], 'must be at least 2'),
                                       (['--quantile', '--qr_kappa=0'], 'must be > 0'),
                                       (['--quantile', '--qr_kappa=-1'], 'must be > 0')])
def test_quantile_flag_errors(argv, word, capsys):
    from dist_dqn_amd.config import parse_args
    with pytest.raises(SystemExit):
        parse_args(argv)
    assert word in capsys.readouterr().err


def test_build_arch_rejects_what_the_flags_reject():
    from dist_dqn_amd.models.arch import build_arch
    for kw in (dict(distributional=True), dict(num_quantiles=1), dict(kappa=0.0)):
        with pytest.raises(RuntimeError):
            build_arch('nature', (84, 84, 4), 6, quantile=True, **kw)


@pytest.mark.parametrize('network,shape', [('nature', (84, 84, 4)), ('cnn', (84, 84, 4)), ('simple', (4,))])
@pytest.mark.parametrize('dueling', [False, True])
def test_quantile_arch_has_the_c51_widths(network, shape, dueling):
    from dist_dqn_amd.models.arch import build_arch
    from dist_dqn_amd.models.params import FlatLayout
    for n in (2, 32, 51, 64):
        q = build_arch(network, shape, 6, dueling=dueling, quantile=True, num_quantiles=n, kappa=0.5, noisy=True)
        c = build_arch(network, shape, 6, dueling=dueling, distributional=True, num_atoms=n, noisy=True)
        assert q.quantile and q.kappa == 0.5 and q.distributional and q.atoms == n == c.atoms
        assert not c.quantile and q.dueling == c.dueling == dueling
        assert q.param_specs() == c.param_specs() and q.head == c.head and q.value == c.value
        lq, lc = FlatLayout(q), FlatLayout(c)
        assert lq.offsets == lc.offsets and lq.total == lc.total
    plain = build_arch(network, shape, 6, dueling=dueling)
    assert not plain.quantile and not plain.distributional


def test_arch_from_config_and_executor_support():
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.models.arch import arch_from_config
    from dist_dqn_amd.ops.executor import supports
    a = arch_from_config(parse_args(['--network=nature', '--quantile', '--num_quantiles=64', '--qr_kappa=2']),
                         (84, 84, 4), 6)
    assert a.quantile and a.atoms == 64 and a.kappa == 2.0 and supports(a)
    b = arch_from_config(parse_args(['--network=nature', '--quantile', '--num_quantiles=65']), (84, 84, 4), 6)
    assert b.quantile and b.atoms == 65 and not supports(b)
    c = arch_from_config(parse_args(['--network=nature', '--distributional']), (84, 84, 4), 6)
    assert not c.quantile and c.atoms == 51


# ------------------------------------------------------------------ a few steps on the CPU
def test_simple_quantile_net_trains_on_the_cpu():
    """A CartPole-sized `simple` net, dueling + Double DQN, on one fixed batch: finite losses that
    do not grow (a smoke check of the wiring, not a learning claim); Q = mean of the quantiles."""
    from dist_dqn_amd.config import parse_args
    from dist_dqn_amd.models import torch_net
    from dist_dqn_amd.models.network import Network
    cfg = parse_args(['--device=cpu', '--seed=1', '--network=simple', '--quantile', '--num_quantiles=8', '--dueling',
                      '--double_dqn', '--optimizer=adam', '--lr=0.01', '--reg_param=0'])
    net = Network.create_network(cfg, (4,), 2)
    assert net.executor.name == 'torch' and net.arch.quantile
    g = torch.Generator().manual_seed(3)
    n = 16
    batch = {'states': torch.randn(n, 4, generator=g), 'next_states': torch.randn(n, 4, generator=g),
             'actions': torch.randint(0, 2, (n,), generator=g), 'rewards': torch.randn(n, generator=g),
             'dones': (torch.rand(n, generator=g) < 0.3).float(), 'gammas': torch.full((n,), 0.9)}
    losses = []
    for _ in range(8):
        loss, prio = net.train_step(batch)
        assert prio.shape == (n,) and torch.isfinite(prio).all() and (prio >= 0).all()
        losses.append(float(loss))
    assert np.isfinite(losses).all() and losses[-1] <= losses[0] * (1.0 + 1e-3), losses
    out = torch_net.forward(net.arch, net.online.flat, net.layout, batch['states'])
    assert out.shape == (n, 2, 8)
    torch.testing.assert_close(net.q_values(batch['states']), out.mean(-1))
    torch.testing.assert_close(torch_net.q_from_output(net.arch, out), out.mean(-1))
