"""TD losses (torch oracle; the fused HIP kernel is `csrc/kernels/td_loss.hip`).

Reference loss (`/root/reference/src/network.py:141-157`, targets built on
the host at `/root/reference/src/dqn_agent.py:224-253`):
    y  = r + gamma * max_a' Q_target(s', a')   (y = r when terminal)
    L  = mean((Q(s, a) - y)^2) + reg_param * sum_w 0.5 ||w||^2
Extensions: Huber, Double DQN (argmax by the online net), n-step discount
(gamma_n = gamma ** n), importance weights (PER), the C51 categorical
projection loss, the QR-DQN quantile regression loss and the Munchausen-DQN
soft target (``munchausen_loss``). The L2 term is NOT
part of these functions: it is applied as ``grad += reg_param * w`` in the
optimizer (same gradient, no extra pass).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def elementwise(d: torch.Tensor, kind: str, delta: float = 1.0) -> torch.Tensor:
    if kind == 'mse':
        return d * d
    if kind == 'huber':
        ad = d.abs()
        return torch.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta))
    raise ValueError(kind)


def scalar_td_loss(q: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor,
                   dones: torch.Tensor, q_next_target: torch.Tensor,
                   q_next_online: Optional[torch.Tensor] = None, gamma: float = 0.99,
                   kind: str = 'mse', delta: float = 1.0,
                   weights: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (loss, |td_error|). ``q_next_online`` given => Double DQN."""
    a = actions.long().view(-1, 1)
    q_sa = q.gather(1, a).squeeze(1)
    with torch.no_grad():
        sel = q_next_online if q_next_online is not None else q_next_target
        a_star = sel.argmax(dim=1, keepdim=True)
        nxt = q_next_target.gather(1, a_star).squeeze(1)
        y = rewards.float() + gamma * (1.0 - dones.float()) * nxt
    d = q_sa - y
    per = elementwise(d, kind, delta)
    if weights is not None:
        per = per * weights
    return per.mean(), d.detach().abs()


def categorical_projection(p_next: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor,
                           gamma: float, v_min: float, v_max: float) -> torch.Tensor:
    """Project r + gamma*z onto the fixed support (Bellemare et al. 2017). p_next: [B, N]."""
    B, N = p_next.shape
    z = torch.linspace(v_min, v_max, N, device=p_next.device)
    dz = (v_max - v_min) / (N - 1)
    tz = (rewards.float().view(B, 1) + gamma * (1.0 - dones.float().view(B, 1)) * z.view(1, N))
    tz = tz.clamp(v_min, v_max)
    top = float(torch.tensor(v_max, dtype=tz.dtype))        # v_max as tz holds it (host scalar)
    # fp32 (v_max - v_min) / dz is not always N - 1 (61.000004 for [-1, 1] with 62 atoms: the
    # ceil neighbour would be index N; 62.999996 for [-10, 10] with 64: a target clamped to
    # v_max would leak mass to atom N - 2), so, as the HIP kernels do, a clamped target sits on
    # the last atom exactly and nothing lies beyond it
    b = ((tz - v_min) / dz).clamp(max=N - 1).masked_fill(tz >= top, N - 1)
    lo = b.floor().long()
    hi = b.ceil().long()
    m = torch.zeros(B, N, device=p_next.device)
    eq = (lo == hi).float()
    m.scatter_add_(1, lo, p_next * (hi.float() - b + eq))
    m.scatter_add_(1, hi, p_next * (b - lo.float()))
    return m


def c51_loss(logits: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor,
             dones: torch.Tensor, logits_next_target: torch.Tensor,
             logits_next_online: Optional[torch.Tensor], gamma: float, v_min: float,
             v_max: float, weights: Optional[torch.Tensor] = None):
    """logits: [B, A, N]. Returns (loss, per-sample cross-entropy)."""
    B, A, N = logits.shape
    z = torch.linspace(v_min, v_max, N, device=logits.device)
    with torch.no_grad():
        p_t = torch.softmax(logits_next_target.float(), dim=-1)
        sel = logits_next_online if logits_next_online is not None else logits_next_target
        q_sel = (torch.softmax(sel.float(), dim=-1) * z).sum(-1)
        a_star = q_sel.argmax(dim=1)
        p_next = p_t[torch.arange(B, device=logits.device), a_star]
        m = categorical_projection(p_next, rewards, dones, gamma, v_min, v_max)
    logp = F.log_softmax(logits.float(), dim=-1)[torch.arange(B, device=logits.device), actions.long()]
    per = -(m * logp).sum(-1)
    pr = per.detach().clone()
    if weights is not None:
        per = per * weights
    return per.mean(), pr


def qr_loss(theta: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor,
            theta_next_target: torch.Tensor, theta_next_online: Optional[torch.Tensor], gamma, kappa: float,
            weights: Optional[torch.Tensor] = None):
    """Quantile regression loss (QR-DQN, Dabney et al. 2018). theta: [B, A, N] quantile values at
    the midpoints tau_i = (2i + 1) / 2N. gamma: float or per-row [B] / [B, 1]. Returns (loss,
    per-sample loss before the importance weights: the PER priority).

    a* = argmax_a mean_j theta_sel(s', a)_j (first maximum; sel = online net under Double DQN),
    u_ij = r + gamma (1 - done) theta_target(s', a*)_j - theta(s, a)_i,
    per = sum_i mean_j |tau_i - 1{u_ij < 0}| L_kappa(u_ij) / kappa (L_kappa: Huber)."""
    B, A, N = theta.shape
    rows = torch.arange(B, device=theta.device)
    with torch.no_grad():
        sel = theta_next_online if theta_next_online is not None else theta_next_target
        a_star = sel.float().mean(-1).argmax(dim=1)
        g = torch.as_tensor(gamma, dtype=torch.float32, device=theta.device).reshape(-1, 1)
        tz = rewards.float().view(B, 1) + g * (1.0 - dones.float().view(B, 1)) * theta_next_target.float()[rows, a_star]
        tau = (2.0 * torch.arange(N, device=theta.device, dtype=torch.float32) + 1.0) / (2.0 * N)
    th = theta.float()[rows, actions.long()]                       # [B, N]
    u = tz.view(B, 1, N) - th.view(B, N, 1)                         # [B, i, j]
    rho = (tau.view(1, N, 1) - (u.detach() < 0).float()).abs() * elementwise(u, 'huber', kappa) / kappa
    per = rho.mean(2).sum(1)
    pr = per.detach().clone()
    if weights is not None:
        per = per * weights
    return per.mean(), pr


def munchausen_loss(q: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor,
                    q_next_target: torch.Tensor, q_target: torch.Tensor, gamma, alpha: float = 0.9,
                    tau: float = 0.03, clip: float = -1.0, kind: str = 'mse', delta: float = 1.0,
                    weights: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Munchausen-DQN loss (Vieillard, Pietquin, Geist 2020). q: online Q(s, .) [B, A];
    q_next_target / q_target: the TARGET net on s' and on s. gamma: float or per-row [B] (it
    carries the n-step power; the bonus is that of the sampled (s, a) only). Returns (loss,
    |td_error|). With pi = softmax(q_target_net / tau), in max-subtracted form (finite for
    tau = 0.03 and Q values of a few hundred):

        lp(x, a) = q(x, a) - max_k q(x, k) - tau log sum_k exp((q(x, k) - max_k q(x, k)) / tau)   (= tau log pi, <= 0)
        soft(x)  = max_k q(x, k) + tau log sum_k exp((q(x, k) - max_k q(x, k)) / tau)
        y        = r + alpha clip(lp(s, a), l0, 0) + gamma (1 - done) soft(s')
        td       = y - Q(s, a)

    The per-sample loss, weights and reduction are ``scalar_td_loss``'s; y carries no gradient."""
    a = actions.long().view(-1, 1)
    q_sa = q.gather(1, a).squeeze(1)
    with torch.no_grad():
        qn, qs = q_next_target.float(), q_target.float()
        mn, ms = qn.max(dim=1, keepdim=True).values, qs.max(dim=1, keepdim=True).values
        soft = mn.squeeze(1) + tau * torch.log(torch.exp((qn - mn) / tau).sum(1))
        lse = tau * torch.log(torch.exp((qs - ms) / tau).sum(1))
        lp = (qs - ms).gather(1, a).squeeze(1) - lse
        g = torch.as_tensor(gamma, dtype=torch.float32, device=q.device).reshape(-1)
        y = rewards.float() + alpha * lp.clamp(clip, 0.0) + g * (1.0 - dones.float()) * soft
    d = q_sa - y
    per = elementwise(d, kind, delta)
    if weights is not None:
        per = per * weights
    return per.mean(), d.detach().abs()
