"""Test helper: the seeded inputs and the float64 reference of the QR-DQN heads, shared by the
narrow head's tests (test_qr_head_gpu.py, whose docstring states the reference and derives the
bounds), the wide head's (test_qr_wide_head_gpu.py) and the acting tests (test_qr_acting_gpu.py).
"""
import numpy as np
import torch

import head_ref as hr
from head_ref import E24, HID, PAD_IN, dims


# ------------------------------------------------------------------ inputs (CPU, seeded)
def inputs(B, A, N, dueling, double, wmode, kappa, seed):
    g = torch.Generator().manual_seed(seed)
    NO, VO, KD = dims(A, N, dueling)
    x = torch.randn(3, B, A, N, generator=g)
    v = torch.randn(3, B, N, generator=g)
    tie = None
    if B > 8:
        x[:, 8] *= 30.0
        v[:, 8] *= 30.0
    if B > 9 and double:
        # two actions of the selection instance bit-identical and (shifted up) the greedy ones;
        # the target's rows of the two differ, so the later maximum shows
        i1, i2 = A // 3, A - 1
        x[2, 9, i1] += 6.0
        x[2, 9, i2] = x[2, 9, i1]
        tie = (9, i1, i2)
    rew, done, gam = hr.draw_transitions(g, B, [(1.0, 1.0, 0.99), (0.5, 0.0, 0.0)])
    act = hr.draw_actions(g, B, A)
    wts, zrow = hr.draw_weights(g, B, wmode)
    rows = torch.full((3, B, KD), PAD_IN)
    rows[:, :, :NO] = x.reshape(3, B, NO)
    if dueling:
        rows[:, :, VO:VO + N] = v
    return dict(B=B, A=A, N=N, dueling=dueling, double=double, kappa=kappa, rows=rows.float(), rew=rew, done=done,
                gam=gam, act=act, wts=wts, tie=tie, zrow=zrow)


def seed(B, A, N, dueling, double):
    return 1000 * A + 10 * N + B + 2 * dueling + double


_cache = {}


def case(key):
    """(inputs, float64 reference) of a case (B, A, N, dueling, double, weights, kappa): computed
    once, shared, never modified."""
    if key not in _cache:
        B, A, N, dueling, double, wmode, kappa = key
        c = inputs(B, A, N, dueling, double, wmode, kappa, seed(B, A, N, dueling, double))
        _cache[key] = (c, reference(c))
    return _cache[key]


# ------------------------------------------------------------------ float64 reference
def quantiles64(rows, A, N, dueling):
    """Quantiles [.., A, N] (dueling combined) of output rows [.., KD], and the largest |input| [..]."""
    NO, VO, _ = dims(A, N, dueling)
    r = rows.double().numpy()
    x = r[..., :NO].reshape(r.shape[:-1] + (A, N))
    mag = np.abs(r[..., :NO]).max(-1)
    if dueling:
        mag = np.maximum(mag, np.abs(r[..., VO:VO + N]).max(-1))
        x = x + r[..., None, VO:VO + N] - x.mean(-2, keepdims=True)
    return x, mag


def reference(c):
    B, A, N, k = c['B'], c['A'], c['N'], float(c['kappa'])
    th, mag = quantiles64(c['rows'], A, N, c['dueling'])      # [3, B, A, N], [3, B]
    q = th.mean(-1)                                           # [3, B, A]
    s = 2 if c['double'] else 1
    qs = q[s]
    best = np.zeros(B, dtype=np.int64)
    for b in range(B):
        for i in range(1, A):
            if qs[b, i] > qs[b, best[b]]:                     # strictly greater: the first maximum wins
                best[b] = i
    top = np.sort(qs, axis=1)
    rng = th[s].reshape(B, -1).max(-1) - th[s].reshape(B, -1).min(-1)
    skip = (top[:, -1] - top[:, -2]) < 1e-4 * rng
    if c['tie'] is not None:
        b, i1, i2 = c['tie']
        assert qs[b, i1] == qs[b, i2] == qs[b].max() and best[b] == i1
        skip[b] = False
    r, d, gm = (c[n].double().numpy() for n in ('rew', 'done', 'gam'))
    T = r[:, None] + (gm * (1.0 - d))[:, None] * th[1][np.arange(B), best]         # [B, N]
    act = c['act'].long().numpy()
    on = th[0][np.arange(B), act]                                                  # [B, N]
    u = T[:, None, :] - on[:, :, None]                                             # [B, i, j]
    tau = ((2 * np.arange(N) + 1) / (2.0 * N))[None, :, None]
    wq = np.abs(tau - (u < 0))
    au = np.abs(u)
    hub = np.where(au <= k, 0.5 * u * u, k * (au - 0.5 * k))
    per = (wq * hub / k).mean(2).sum(1)
    g = -(wq * np.clip(u, -k, k) / k).mean(2)                                      # [B, N]
    w = np.ones(B) if c['wts'] is None else c['wts'].double().numpy()
    M = np.maximum(np.maximum(mag[0], mag[1]), np.maximum(np.abs(T).max(-1), np.abs(on).max(-1)))
    return dict(q=q, mag=mag, best=best, skip=skip, per=per, w=w, g=g, M=M)


def dout_ref(c, ref):
    """(g [B, KD] before the w / B factor, |dueling coefficient| [B, KD], written-column mask [KD])."""
    B, A, N = c['B'], c['A'], c['N']
    NO, VO, KD = dims(A, N, c['dueling'])
    g, cf = np.zeros((B, KD)), np.zeros((B, KD))
    onehot = np.eye(A)[c['act'].long().numpy()]               # [B, A]
    coef = onehot - (1.0 / A if c['dueling'] else 0.0)
    g[:, :NO] = (coef[:, :, None] * ref['g'][:, None, :]).reshape(B, NO)
    cf[:, :NO] = np.repeat(np.abs(coef), N, axis=1)
    mask = np.zeros(KD, dtype=bool)
    mask[:NO] = True
    if c['dueling']:
        g[:, VO:VO + N] = ref['g']
        cf[:, VO:VO + N] = 1.0
        mask[VO:VO + N] = True
    return g, cf, mask


def t_g(c, ref):
    """fp32 error bound of g_i per row (test_qr_head_gpu.py's docstring)."""
    du = (2 * (c['A'] + 2) + 2 if c['dueling'] else 2) * E24 * ref['M']
    return du / float(c['kappa']) + (c['N'] + 4) * E24


# ------------------------------------------------------------------ launches
def _call(fn_name, c):
    return fn_name, [c['B'], c['A'], HID, int(c['dueling']), 0, 0], [c['N']], [float(c['kappa'])]


def train(ext, fn_name, c, act_t):
    return hr.train(ext, *_call(fn_name, c), c, act_t, 3 if c['double'] else 2, dims(c['A'], c['N'], c['dueling'])[2])


def check_train(variant, key, fn_name, nb, ratios):
    c, ref = case(key)
    g, cf, mask = dout_ref(c, ref)
    hr.check_train(variant, c, _call(fn_name, c), 3 if c['double'] else 2, mask.size, nb,
                   dict(g=g, t=t_g(c, ref)[:, None] * cf, mask=mask, prio=ref['per'], per=ref['per'], w=ref['w'],
                        skip=ref['skip']), ('per', 'per', 'a quantile / value column'), ratios)


def check_near_tie_cap(keys):
    """No GPU: the reference alone."""
    for key in keys:
        c, ref = case(key)
        assert int(ref['skip'].sum()) * 16 <= c['B'], (key, np.nonzero(ref['skip'])[0])
        assert c['tie'] is None or not ref['skip'][c['tie'][0]]
        assert (ref['per'] >= 0).all() and (np.abs(ref['g']) <= 1.0).all()


def check_infer(fn_name, B, A, N, dueling):
    """q_values' kernel: Q = mean over quantiles, within (3 N + A + 4) e M (dueling) / (N + 2) e M."""
    c = inputs(B, A, N, dueling, False, 'none', 1.0, seed(B, A, N, dueling, 0))
    q = hr.infer(hr.ext(''), fn_name, [N], [1.0], c['rows'][0], B, A, dueling)
    th, mag = quantiles64(c['rows'][0], A, N, dueling)
    err = np.abs(q - th.mean(-1))
    bound = ((3 * N + A + 4) if dueling else (N + 2)) * E24 * mag[:, None]
    print('q: max err / bound %.3f' % (err / bound).max())
    assert (err <= bound).all(), float((err / bound).max())
