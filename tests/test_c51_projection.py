"""The torch oracle's categorical projection (``models/losses.py``) against a float64 reference
in closed form (no floor / ceil, so nothing to index):

    m_i = sum_j p_j * clip(1 - |clamp(r + g z_j, v_min, v_max) - z_i| / dz, 0, 1)

on supports whose fp32 ``(v_max - v_min) / dz`` lands on ``N - 1`` and on supports where it
rounds above it ((-1, 1, 62): 61.000004) -- there the ceil neighbour of a target clamped to
``v_max`` used to be index N. Every batch starts with the projection's edge rows (terminal
rewards beyond either end, on ``v_max``, on atoms; the identity projection; half a bin; gamma 0).
"""
import numpy as np
import pytest
import torch

from dist_dqn_amd.models import losses

SUPPORTS = [(-10.0, 10.0, 51), (-10.0, 10.0, 64), (0.0, 200.0, 21), (0.0, 1.0, 2),
            (-1.0, 1.0, 62), (-21.0, 21.0, 30), (-3.7, 11.3, 54)]     # the last three overflow in fp32


def _rows(v_min, v_max, N, B, seed):
    """(p [B, N], rewards, dones, gammas) as fp32: the edge rows, then random ones."""
    g = torch.Generator().manual_seed(seed)
    dz = (v_max - v_min) / (N - 1)
    z = torch.linspace(v_min, v_max, N)
    edges = [(v_max + 1.0, 1.0, 0.99), (v_min - 1.0, 1.0, 0.99), (v_max, 1.0, 0.99), (0.0, 1.0, 0.99),
             (float(z[N // 3]), 1.0, 0.99), (0.0, 0.0, 1.0), (dz / 2, 0.0, 1.0),
             (v_min + 0.3 * (v_max - v_min), 0.0, 0.0)]
    n = B - len(edges)
    r = torch.cat([torch.tensor([e[0] for e in edges]), torch.randn(n, generator=g) * (v_max - v_min) / 4])
    d = torch.cat([torch.tensor([e[1] for e in edges]), (torch.rand(n, generator=g) < 0.2).float()])
    gm = torch.cat([torch.tensor([e[2] for e in edges]), torch.tensor([0.99 ** (1 + i % 3) for i in range(n)])])
    p = torch.softmax(torch.randn(B, N, generator=g) * 2.0, dim=-1)
    return p.float(), r.float(), d.float(), gm.float()


def _project64(p, r, d, gm, v_min, v_max):
    p, r, d, gm = (t.double().numpy() for t in (p, r, d, gm))
    N = p.shape[1]
    z = np.linspace(v_min, v_max, N)
    dz = (v_max - v_min) / (N - 1)
    tz = np.clip(r[:, None] + (gm * (1.0 - d))[:, None] * z[None, :], v_min, v_max)          # [B, j]
    k = np.clip(1.0 - np.abs(tz[:, :, None] - z[None, None, :]) / dz, 0.0, 1.0)              # [B, j, i]
    return (p[:, :, None] * k).sum(1)


@pytest.mark.parametrize('v_min,v_max,N', SUPPORTS)
def test_categorical_projection_matches_float64(v_min, v_max, N):
    p, r, d, gm = _rows(v_min, v_max, N, 40, seed=N)
    ref = _project64(p, r, d, gm, v_min, v_max)
    np.testing.assert_allclose(ref.sum(1), p.double().sum(1).numpy(), rtol=0, atol=1e-12)   # (it keeps the mass)
    m = losses.categorical_projection(p, r, d, gm.view(-1, 1), v_min, v_max)
    assert m.shape == p.shape
    err = np.abs(m.double().numpy() - ref)
    print('max |m - ref| %.3g, max |mass - 1| %.3g' % (err.max(), float((m.double().sum(1) - 1).abs().max())))
    assert err.max() <= 1e-5, (err.max(), np.unravel_index(err.argmax(), err.shape))
    assert float((m.double().sum(1) - 1).abs().max()) <= 1e-5


def test_categorical_projection_scalar_gamma():
    """The scalar-gamma call of the production torch backend, on an overflowing support."""
    v_min, v_max, N = -1.0, 1.0, 62
    p, r, d, _ = _rows(v_min, v_max, N, 24, seed=1)
    gm = torch.full((24,), 0.99)
    ref = _project64(p, r, d, gm, v_min, v_max)
    m = losses.categorical_projection(p, r, d, 0.99, v_min, v_max)
    assert np.abs(m.double().numpy() - ref).max() <= 1e-5


def test_c51_loss_runs_on_overflowing_support():
    """Forward and backward on (-1, 1, 62) (raised ``index 62 is out of bounds`` before the clamp);
    the per-sample cross-entropy agrees with the float64 projection."""
    v_min, v_max, N, B, A = -1.0, 1.0, 62, 24, 3
    _, r, d, gm = _rows(v_min, v_max, N, B, seed=2)
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(B, A, N, generator=g, requires_grad=True)
    lt, lo = torch.randn(B, A, N, generator=g), torch.randn(B, A, N, generator=g)
    act = torch.randint(0, A, (B,), generator=g)
    w = torch.rand(B, generator=g) + 0.5
    loss, prio = losses.c51_loss(lg, act, r, d, lt, lo, gm.view(-1, 1), v_min, v_max, w)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(lg.grad).all()
    z = torch.linspace(v_min, v_max, N)
    a_star = (torch.softmax(lo, -1) * z).sum(-1).argmax(1)
    p_next = torch.softmax(lt, -1)[torch.arange(B), a_star]
    m = _project64(p_next, r, d, gm, v_min, v_max)
    logp = torch.log_softmax(lg.detach().double(), -1)[torch.arange(B), act].numpy()
    ce = -(m * logp).sum(1)
    np.testing.assert_allclose(prio.numpy(), ce, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(loss.detach()), float((ce * w.double().numpy()).mean()), rtol=1e-4, atol=1e-5)
