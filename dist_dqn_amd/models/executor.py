"""Executors: how a Q-network's forward / loss+gradient is computed.

`TorchExecutor` — PyTorch ops + autograd over the flat buffer (CPU path and
numerics oracle). The fused HIP executor lives in `dist_dqn_amd/ops/executor.py`
and implements the same two methods with hand-written CDNA4 kernels.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import torch_net
from .arch import ArchSpec
from .params import FlatLayout


def check_munchausen(arch: ArchSpec, double_dqn: bool, alpha: float, tau: float, clip: float):
    """The combinations and ranges every executor accepts for a Munchausen-DQN target."""
    if arch.distributional or double_dqn:
        raise RuntimeError('munchausen: a scalar Q-network without double_dqn (the target is a softmax over the '
                           'target net\'s Q values: no return distribution, no argmax to decouple)')
    if not (0.0 <= alpha <= 1.0 and tau > 0.0 and clip < 0.0):
        raise RuntimeError('munchausen: 0 <= m_alpha <= 1, m_tau > 0, m_clip < 0; got %g, %g, %g' % (alpha, tau, clip))


class TorchExecutor:
    name = 'torch'
    compute_dtype = 'fp32'

    def __init__(self, arch: ArchSpec, layout: FlatLayout, input_scale: float = 1.0,
                 loss: str = 'mse', huber_delta: float = 1.0, double_dqn: bool = False, oracle: bool = False,
                 munchausen: Optional[Tuple[float, float, float]] = None):
        """munchausen = (alpha, tau, clip): the Munchausen-DQN target (losses.munchausen_loss), which
        also runs the target net on the sampled states. oracle=True: every op in PyTorch, the TD loss included (the numerics reference the HIP
        kernels are tested against); otherwise the TD loss on cuda tensors runs the fused
        td_loss kernel (the `simple` MLP's GPU training path)."""
        self.arch, self.layout = arch, layout
        self.input_scale = input_scale
        self.loss_kind, self.delta, self.double = loss, huber_delta, double_dqn
        self.oracle = bool(oracle)
        self.munchausen = None if munchausen is None else tuple(float(v) for v in munchausen)
        if self.munchausen is not None:
            check_munchausen(arch, double_dqn, *self.munchausen)

    def forward(self, flat: torch.Tensor, x: torch.Tensor, noise: Optional[torch.Tensor] = None):
        with torch.no_grad():
            return torch_net.forward(self.arch, flat, self.layout, x, self.input_scale, noise)

    def q_values(self, flat, x, noise=None):
        return torch_net.q_from_output(self.arch, self.forward(flat, x, noise))

    def loss_and_grad(self, online: torch.Tensor, target: torch.Tensor, batch: Dict[str, torch.Tensor],
                      grad_out: torch.Tensor, noise: Optional[torch.Tensor] = None,
                      noise_target: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Writes dLoss/dflat into grad_out; returns (loss [1], |td|, CE or quantile loss per sample [B])."""
        arch = self.arch
        flat = online.detach().requires_grad_(True)
        out = torch_net.forward(arch, flat, self.layout, batch['states'], self.input_scale, noise)
        with torch.no_grad():
            nt = torch_net.forward(arch, target, self.layout, batch['next_states'], self.input_scale, noise_target)
            no = (torch_net.forward(arch, online, self.layout, batch['next_states'], self.input_scale, noise)
                  if self.double else None)
            # Munchausen-DQN: the target net on s as well (the log-policy bonus of the sampled action)
            ts = (torch_net.forward(arch, target, self.layout, batch['states'], self.input_scale, noise_target)
                  if self.munchausen is not None else None)
        from ..ops.td import td_loss
        loss, prio = td_loss(out, batch['actions'], batch['rewards'], batch['dones'], batch['gammas'], nt, no,
                             batch.get('weights'), self.loss_kind, self.delta, arch.distributional,
                             arch.v_min, arch.v_max, pure_torch=self.oracle,
                             kappa=arch.kappa if arch.quantile else None, munchausen=self.munchausen, q_target=ts)
        g, = torch.autograd.grad(loss, flat)
        grad_out.copy_(g)
        return loss.detach().view(1), prio
