"""The Munchausen-DQN head kernels (csrc/kernels/mdqn_head.hip: mdqn_train_kernel,
mdqn_infer_kernel) against a float64 reference of the same operation, at the shapes where the
kernels change path.

As in test_qr_head_gpu.py the binding takes the output rows as pointers, so the kernels run on
synthetic fp32 rows with no network: ``KD`` floats = [A values | pad to 32 | dueling value at
VO = 32 | pad to 64] (KD = 32 without dueling), three instances: online(s), target(s'),
target(s). The input pads hold 1e9 (a kernel that read one would show it) and the outputs start
as a sentinel (a written pad column would show).

Reference (numpy float64, on the fp32 input values; nothing from ``models/losses.py``): dueling
combine Q = A + V - mean A on all three rows, soft = max q' + tau log sum exp((q' - max q') / tau),
lp = q0_a - max q0 - tau log sum exp((q0 - max q0) / tau), y = r + alpha clip(lp, l0, 0) +
gamma (1 - done) soft, d = Q_a - y, prio = |d|, per = d^2 or Huber_delta(d), g = 2 d or
clamp(d, -delta, delta); dL/dQ = w / B g (dueling: advantage columns times (i == a) - 1 / A, the
value column plain).

Cases. The kernel has no template instances: lanes [0, 32) and [32, 64) of a wave hold the
actions of two instances, reduced on 16-lane DPP rows. Its width boundaries are therefore the DPP
row (A = 16 | 17: the second row of a half-wave comes into use) and the half-wave (A = 32); the
action counts 2, 4, 5, 8, 9, 16, 17, 18, 19, 32 cover both sides of each. B = 1, 8, 9, 24 and
513 (the block-stride loop: 64 blocks of eight waves take 512 samples a pass); plain / dueling;
MSE and Huber (delta 1 and 0.5); weights absent, random, containing an exact 0; tau 0.03 and 1;
alpha 0.9 and 0. Row 0 is terminal, row 1 has gamma = 0, a fifth of the rest are terminal; row 8
is scaled by 30 (Q range about 100: at tau = 0.03 the exponents reach -3000, and lp falls far
below l0: the max-subtraction and the clip); row 9 has two bit-identical maximal actions in both
target rows, one of them the taken action.

Bounds. ``prio`` and the loss: rtol 1e-4, atol 1e-5 (the C51 / QR head tests' bound for a
per-sample fp32 reduction). ``dout16`` elementwise: |err| <= (ulp + 5 e) |ref| + t, ulp = 2^-8
(bf16), 2^-11 (fp16), 0 (fp32) the storage step, 5 e the roundings of w / B, its products with g,
the loss scale and the dueling coefficient, and t = t_g |coef| w_b / B times the fp16 build's
loss scale, with t_g the fp32 error of g, derived with e = 2^-24, M the row's largest |input|:
  * a combined Q (dueling): the action sum on a 5-level tree, its scaling by the rounded 1 / A,
    v - mean, x + (v - mean) with results up to 3 M: dq = 13 e M, |Q| <= Mq = 3 M; plain: dq = 0,
    Mq = M;
  * log-sum-exp is 1-Lipschitz in the sup norm, so the exact soft / lse of the computed Q moves
    by <= dq; its fp32 evaluation: z_k = (q_k - m) / tau carries a relative 2 e, which moves
    exp(z_k) by <= |z_k| exp(z_k) 2 e <= 0.74 e; expf (the accurate library function, budgeted
    at 2 ulp = 4 e relative), the 6-level sum S >= 1 (the maximum's term is exactly 1): dS / S <=
    (10 + 0.74 A) e; logf (2 ulp of a result <= log 32: 8 e), the product with tau and the sum
    with m: d_soft <= dq + e (Mq + tau log A) + tau (22 + 0.74 A) e;
  * lp = (q0_a - m0) - tau log S0 is 2-Lipschitz: d_lp <= 2 dq + e (4 Mq + tau log A) +
    tau (22 + 0.74 A) e; the clip is 1-Lipschitz (continuous at l0 and at 0: no exclusion);
  * y and d = Q_a - y: the products with alpha <= 1 and gamma (1 - done) <= 1 (relative 2 e),
    two sums and the difference, each rounding a result <= |r| + |l0| + 2 Mq + tau log A:
    t_d = e (52 M [dueling] + 10 Mq + 3 |r| + 4 |l0| + tau (44 + 1.5 A + 6 log A));
  * g = 2 d exactly (MSE): t_g = 2 t_d; Huber: clamp is 1-Lipschitz and continuous at the knee:
    t_g = t_d.
No case or row is excluded (the target has no argmax): the test has no row mask and asserts that
the compared elements number B (A + dueling).

Q of the inference kernel: plain rows are copied (exact); dueling: the 5-level action sum, its
division by A, v - mean, x + (v - mean): 11 e M.

Largest observed err / bound over all cases of the build (one MI355X run): bf16 0.964 and fp16
0.788 (the storage rounding: round-to-nearest reaches the full step at the bottom of a binade),
fp32 0.011; dueling Q of the inference kernel 0.240 of 11 e M, plain Q exact. Largest |err| of
``prio`` 1.4e-5 at |td| up to 294.
"""
import numpy as np
import pytest
import torch

import head_ref as hr
from head_ref import DEV, E24, HID, PAD_IN, ext as _ext

FN = 'qnet_mdqn_head'
VO = 32


def _kd(dueling):
    return 64 if dueling else 32


def _blocks(B):
    return min((B + 7) // 8, 64)


# ------------------------------------------------------------------ inputs (CPU, seeded)
def _inputs(B, A, dueling, huber, delta, wmode, tau, alpha, seed, clip=-1.0):
    g = torch.Generator().manual_seed(seed)
    KD = _kd(dueling)
    x = torch.randn(3, B, A, generator=g) * 3.0
    v = torch.randn(3, B, generator=g) * 3.0
    act = hr.draw_actions(g, B, A)
    tie = None
    if B > 8:
        x[:, 8] *= 30.0
        v[:, 8] *= 30.0
        act[8] = int(x[2, 8].argmin())
        x[2, 8, act[8]] = x[2, 8].max() - 60.0  # far below the target's maximum: lp << l0
    if B > 9:
        i1, i2 = A // 3, A - 1
        for inst in (1, 2):
            x[inst, 9, i1] = x[inst, 9].max() + 2.0
            x[inst, 9, i2] = x[inst, 9, i1]
        act[9] = i2
        tie = (9, i1, i2)
    rew, done, gam = hr.draw_transitions(g, B, [(1.0, 1.0, 0.99), (0.5, 0.0, 0.0)])
    wts, zrow = hr.draw_weights(g, B, wmode)
    rows = torch.full((3, B, KD), PAD_IN)
    rows[:, :, :A] = x
    if dueling:
        rows[:, :, VO] = v
    return dict(B=B, A=A, dueling=dueling, huber=huber, delta=delta, tau=tau, alpha=alpha, clip=clip,
                rows=rows.float(), rew=rew, done=done, gam=gam, act=act, wts=wts, tie=tie, zrow=zrow)


# ------------------------------------------------------------------ float64 reference
def _q64(rows, A, dueling):
    """Q [.., A] (dueling combined) of output rows [.., KD], and the largest |input| [..]."""
    r = rows.double().numpy()
    x = r[..., :A]
    mag = np.abs(x).max(-1)
    if dueling:
        mag = np.maximum(mag, np.abs(r[..., VO]))
        x = x + r[..., VO:VO + 1] - x.mean(-1, keepdims=True)
    return x, mag


def _lse64(q, tau):
    m = q.max(-1)
    return m + tau * np.log(np.exp((q - m[..., None]) / tau).sum(-1)), m


def _reference(c):
    B, A, tau = c['B'], c['A'], float(c['tau'])
    q, mag = _q64(c['rows'], A, c['dueling'])                 # [3, B, A], [3, B]
    rows = np.arange(B)
    act = c['act'].long().numpy()
    soft, _ = _lse64(q[1], tau)
    lse0, _ = _lse64(q[2], tau)
    lp = q[2][rows, act] - lse0
    if c['tie'] is not None:
        b, i1, i2 = c['tie']
        assert q[1][b, i1] == q[1][b, i2] == q[1][b].max() and q[2][b, i1] == q[2][b, i2] == q[2][b].max()
    r, d, gm = (c[n].double().numpy() for n in ('rew', 'done', 'gam'))
    y = r + c['alpha'] * np.clip(lp, c['clip'], 0.0) + gm * (1.0 - d) * soft
    td = q[0][rows, act] - y
    ad = np.abs(td)
    if c['huber']:
        k = float(c['delta'])
        per = np.where(ad <= k, 0.5 * td * td, k * (ad - 0.5 * k))
        g = np.clip(td, -k, k)
    else:
        per, g = td * td, 2.0 * td
    w = np.ones(B) if c['wts'] is None else c['wts'].double().numpy()
    M = mag.max(0)
    return dict(q=q, mag=mag, M=M, lp=lp, soft=soft, ad=ad, per=per, g=g, w=w, r=np.abs(r))


def _dout_ref(c, ref):
    """(g [B, KD] before the w / B factor, |dueling coefficient| [B, KD], written-column mask [KD])."""
    B, A = c['B'], c['A']
    KD = _kd(c['dueling'])
    g, cf = np.zeros((B, KD)), np.zeros((B, KD))
    onehot = np.eye(A)[c['act'].long().numpy()]               # [B, A]
    coef = onehot - (1.0 / A if c['dueling'] else 0.0)
    g[:, :A] = coef * ref['g'][:, None]
    cf[:, :A] = np.abs(coef)
    mask = np.zeros(KD, dtype=bool)
    mask[:A] = True
    if c['dueling']:
        g[:, VO] = ref['g']
        cf[:, VO] = 1.0
        mask[VO] = True
    return g, cf, mask


def _t_g(c, ref):
    """fp32 error bound of g per row (see the module docstring)."""
    A, tau, M = c['A'], float(c['tau']), ref['M']
    Mq = 3.0 * M if c['dueling'] else M
    t_d = E24 * ((52.0 * M if c['dueling'] else 0.0) + 10.0 * Mq + 3.0 * ref['r'] + 4.0 * abs(c['clip'])
                 + tau * (44.0 + 1.5 * A + 6.0 * np.log(A)))
    return t_d if c['huber'] else 2.0 * t_d


# ------------------------------------------------------------------ launches
_ratios = {}


def _check_train(variant, c):
    B, A = c['B'], c['A']
    ref = _reference(c)
    g, cf, mask = _dout_ref(c, ref)
    # no row is left out (skip=None), so every written element of every row is compared
    assert int(mask.sum()) == A + int(c['dueling'])
    call = (FN, [B, A, HID, int(c['dueling']), int(c['huber']), 0], [1],
            [float(c['alpha']), float(c['tau']), float(c['clip']), float(c['delta'])])
    # rel = 5 e: the roundings of w / B, its products with g, the loss scale and the dueling coefficient
    hr.check_train(variant, c, call, 3, _kd(c['dueling']), _blocks(B),
                   dict(g=g, t=_t_g(c, ref)[:, None] * cf, mask=mask, prio=ref['ad'], per=ref['per'], w=ref['w'],
                        skip=None), ('prio', 'd', 'a Q / value column'), _ratios, rel=5 * E24)
    # what the scaled row is there for: the clip at l0 is active and soft sits at the maximum
    if B > 8:
        assert ref['lp'].min() < c['clip'] and (ref['lp'] <= 0).all()


TRAIN_CASES = [
    # B, A, dueling, huber, delta, weights, tau, alpha
    (24, 2, 0, 0, 1.0, 'none', 0.03, 0.9), (24, 4, 1, 1, 1.0, 'rand', 0.03, 0.9), (24, 5, 0, 1, 0.5, 'zero', 1.0, 0.9),
    (24, 8, 1, 0, 1.0, 'rand', 0.03, 0.0), (24, 9, 1, 1, 0.5, 'none', 1.0, 0.9), (24, 16, 1, 1, 1.0, 'zero', 0.03, 0.9),
    (24, 17, 0, 0, 1.0, 'rand', 1.0, 0.9), (24, 18, 1, 1, 1.0, 'zero', 0.03, 0.9), (24, 19, 0, 1, 1.0, 'rand', 0.03, 0.0),
    (24, 32, 1, 0, 1.0, 'zero', 1.0, 0.9), (24, 32, 0, 1, 0.5, 'none', 0.03, 0.9),          # the width boundaries
    (24, 6, 1, 1, 1.0, 'rand', 0.03, 0.9), (24, 6, 0, 0, 1.0, 'none', 1.0, 0.0), (24, 6, 1, 0, 1.0, 'zero', 0.03, 0.9),
    (1, 6, 1, 1, 1.0, 'zero', 0.03, 0.9), (8, 6, 0, 1, 0.5, 'rand', 1.0, 0.9), (9, 6, 1, 0, 1.0, 'none', 0.03, 0.9),
    (513, 6, 1, 1, 1.0, 'zero', 0.03, 0.9), (513, 19, 0, 0, 1.0, 'rand', 1.0, 0.9),         # the block-stride loop
]
OTHER_BUILDS_CASE = (24, 6, 1, 1, 1.0, 'zero', 0.03, 0.9)


def _seed(B, A, dueling, huber):
    return 1000 * A + 10 * B + 2 * dueling + huber


def _make(case):
    B, A, dueling, huber, delta, wmode, tau, alpha = case
    return _inputs(B, A, dueling, huber, delta, wmode, tau, alpha, _seed(B, A, dueling, huber))


def test_reference_identities_on_every_case():
    """No GPU: the float64 reference alone, for every case this file launches: soft in
    [max q', max q' + tau log A], lp <= 0, finite at tau = 0.03 on the scaled row."""
    for case in TRAIN_CASES + [OTHER_BUILDS_CASE]:
        c = _make(case)
        ref = _reference(c)
        mx = ref['q'][1].max(-1)
        assert np.isfinite(ref['ad']).all() and np.isfinite(ref['g']).all()
        assert (ref['soft'] >= mx).all() and (ref['soft'] <= mx + c['tau'] * np.log(c['A']) + 1e-12).all()
        assert (ref['lp'] <= 0).all() and (ref['per'] >= 0).all()
        if c['B'] > 8:
            assert ref['lp'][8] < 10.0 * c['clip'] and ref['mag'][:, 8].max() > 30.0
        if c['huber']:
            assert (np.abs(ref['g']) <= c['delta']).all()


@pytest.mark.gpu
@pytest.mark.parametrize('B,A,dueling,huber,delta,wmode,tau,alpha', TRAIN_CASES)
def test_mdqn_train_matches_float64(B, A, dueling, huber, delta, wmode, tau, alpha):
    _check_train('', _make((B, A, dueling, huber, delta, wmode, tau, alpha)))


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['f16', 'f32'])
def test_mdqn_train_other_builds(variant):
    _check_train(variant, _make(OTHER_BUILDS_CASE))


@pytest.mark.gpu
def test_mdqn_head_refuses_bad_arguments():
    """Action count, tau, clip and the inference batch's LDS are checked before any launch."""
    ext = _ext('')
    r = torch.zeros(4, 64, device=DEV)
    q = torch.full((2048 * 32,), float('nan'), dtype=torch.float32, device=DEV)
    io = [0] * 7 + [q.data_ptr()] + [0] * 5
    for A, tau, clip, B, word in ((33, 0.03, -1.0, 4, 'actions'), (6, 0.0, -1.0, 4, 'tau'), (6, 0.03, 0.0, 4, 'clip'),
                                  (32, 0.03, -1.0, 2048, 'too large')):
        with pytest.raises(RuntimeError, match=word):
            ext.qnet_mdqn_head([B, A, HID, 0, 0, 1], [1], [0.9, tau, clip, 1.0], [], [], [], [], [], io, [], [], [],
                               [], [], [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    assert torch.isnan(q).all()


# ------------------------------------------------------------------ inference kernel
INFER_POINTS = [(2, 0), (4, 1), (5, 0), (8, 1), (9, 1), (16, 1), (17, 1), (18, 1), (19, 0), (32, 1), (32, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 32, 513])
@pytest.mark.parametrize('A,dueling', INFER_POINTS)
def test_mdqn_infer_matches_float64(A, dueling, B):
    """q_values' kernel: the dueling combine (B = 513: more rows than the block's 64 row groups
    take in eight passes)."""
    c = _inputs(B, A, dueling, 0, 1.0, 'none', 0.03, 0.9, _seed(B, A, dueling, 0))
    q = hr.infer(_ext(''), FN, [1], [0.9, 0.03, -1.0, 1.0], c['rows'][0], B, A, dueling)
    q64, mag = _q64(c['rows'][0], A, dueling)
    err = np.abs(q - q64)
    bound = (11 if dueling else 0) * E24 * mag[:, None]
    print('q: max err / (11 e M) %.3f' % (err / (11 * E24 * mag[:, None])).max())
    assert (err <= bound).all(), float((err / (11 * E24 * mag[:, None])).max())
