"""DrQ random-shift frame augmentation (``--augment shift``): the definition, in torch.

Replicate-pad a frame stack by ``P`` pixels and take a random crop of the original size
(Kostrikov et al. 2020, "Image Augmentation Is All You Need"; also DrQ-eps, data-efficient
Rainbow, SPR, BBF). For minibatch position ``b`` and ``which`` in {0: ``s``, 1: ``s'``}::

    r  = philox(seed ^ AUG_KEY, ctr, b, which)          (Philox4x32-10 of csrc/kernels/common.h)
    dy = (r.x * (2P + 1) >> 32) - P
    dx = (r.y * (2P + 1) >> 32) - P
    out[b, y, x, c] = in[b, clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1), c]

The frames of a stack share one shift; ``s`` and ``s'`` get independent shifts although they
share frames. ``ctr`` is the learner's ``global_step``, ``seed`` comes from ``aug_seed``.

This module is the reference of the HIP kernel (csrc/kernels/augment.hip, which gathers the
shifted stacks straight from the replay frame ring) and the path every executor that is handed
gathered stacks takes (torch executor, CPU, host replay). The Philox here is exact integer
arithmetic in int64 tensors, so both paths draw the same shifts; ``ctr`` may be a device tensor
(no host sync: the function can be captured into a graph).
"""
from __future__ import annotations

from typing import Tuple, Union

import torch

AUG_KEY = 0x6175676d            # "augm": xor-ed into the seed (the kernel's kAugKey)
MAX_PAD = 16
_M32 = 0xFFFFFFFF


def aug_seed(seed, rank: int = 0) -> int:
    """The augmentation stream's 63-bit seed, derived once from ``--seed`` and the data-parallel
    rank (ranks draw different shifts; the all-reduced gradient keeps the replicas bit-equal)."""
    s = int(seed) if seed is not None else 0
    return (s * 0x9E3779B97F4A7C15 + (int(rank) + 1) * 0xD1B54A32D192ED03 + 0x6175) & 0x7FFFFFFFFFFFFFFF


def _mulhilo(a: int, b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(high, low) 32-bit halves of the 32 x 32 -> 64 bit product a * b (b: int64 holding
    32-bit values), by 16-bit limbs: no intermediate leaves the signed 64-bit range."""
    al, ah = a & 0xFFFF, a >> 16
    bl, bh = b & 0xFFFF, b >> 16
    ll = al * bl
    mid = al * bh + ah * bl + (ll >> 16)
    lo = ((mid & 0xFFFF) << 16) | (ll & 0xFFFF)
    hi = ah * bh + (mid >> 16)
    return hi, lo


def philox(key64: int, ctr_hi: Union[int, torch.Tensor], lo0: torch.Tensor, lo1: torch.Tensor):
    """``philox(key64, ctr_hi, lo0, lo1)`` of common.h on int64 tensors: four tensors (x, y, z, w)
    holding 32-bit values, broadcast over ``lo0`` / ``lo1``. ``ctr_hi``: an int or a one-element
    int64 tensor (its 64 bits are the counter's high words)."""
    key64 = int(key64) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = key64 & _M32, key64 >> 32
    lo0, lo1 = torch.broadcast_tensors(lo0.to(torch.int64), lo1.to(torch.int64))
    c0, c1 = lo0 & _M32, lo1 & _M32
    if torch.is_tensor(ctr_hi):
        ch = ctr_hi.to(device=c0.device, dtype=torch.int64).reshape(-1)[0]
        c2 = (ch & _M32).expand_as(c0)
        c3 = ((ch >> 32) & _M32).expand_as(c0)
    else:
        ch = int(ctr_hi) & 0xFFFFFFFFFFFFFFFF
        c2 = torch.full_like(c0, ch & _M32)
        c3 = torch.full_like(c0, ch >> 32)
    for _ in range(10):
        h0, l0 = _mulhilo(0xD2511F53, c0)
        h1, l1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def check_pad(pad: int) -> int:
    pad = int(pad)
    if not 0 <= pad <= MAX_PAD:
        raise ValueError('augmentation pad must lie in [0, %d], got %d' % (MAX_PAD, pad))
    return pad


def draw_shifts(seed: int, ctr: Union[int, torch.Tensor], B: int, pad: int, device='cpu') -> torch.Tensor:
    """int64 [B, 2, 2]: ``[b, which] = (dy, dx)`` in [-pad, pad]."""
    pad = check_pad(pad)
    dev = torch.device(device)
    b = torch.arange(B, dtype=torch.int64, device=dev).view(B, 1)
    which = torch.arange(2, dtype=torch.int64, device=dev).view(1, 2)
    x, y, _, _ = philox(int(seed) ^ AUG_KEY, ctr, b, which)
    span = 2 * pad + 1
    return torch.stack([((x * span) >> 32) - pad, ((y * span) >> 32) - pad], dim=-1)


def shift(x: torch.Tensor, dydx: torch.Tensor) -> torch.Tensor:
    """``x`` [B, H, W, C] shifted per sample by ``dydx`` [B, 2] with edge replication."""
    assert x.dim() == 4 and tuple(dydx.shape) == (x.shape[0], 2), (tuple(x.shape), tuple(dydx.shape))
    B, H, W, _ = x.shape
    dev = x.device
    d = dydx.to(dev, torch.int64)
    yi = (torch.arange(H, device=dev).view(1, H) + d[:, 0:1]).clamp_(0, H - 1)
    xi = (torch.arange(W, device=dev).view(1, W) + d[:, 1:2]).clamp_(0, W - 1)
    bi = torch.arange(B, device=dev).view(B, 1, 1)
    return x[bi, yi.view(B, H, 1), xi.view(B, 1, W)].contiguous()


def shift_stacks(states: torch.Tensor, next_states: torch.Tensor, seed: int, ctr: Union[int, torch.Tensor],
                 pad: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The augmented minibatch: (s shifted, s' shifted, shifts [B, 2, 2])."""
    if states.dim() != 4:
        raise ValueError('random-shift augmentation needs image states [B, H, W, C], got %s' % (tuple(states.shape),))
    sh = draw_shifts(seed, ctr, states.shape[0], pad, states.device)
    return shift(states, sh[:, 0]), shift(next_states, sh[:, 1]), sh
