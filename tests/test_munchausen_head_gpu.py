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

DEV = torch.device('cuda', 0)
SENT = -4096.0                 # exact in bf16 / fp16 / fp32, below anything the kernels can write
PAD_IN = 1e9
HID = 128                      # (unused by these kernels; the binding wants a multiple of 128)
E24 = 2.0 ** -24
VO = 32
# variant -> (act_t as HipExecutor.act_dtype maps it, storage rounding step, kLossScale)
BUILDS = {'': (torch.bfloat16, 2.0 ** -8, 1.0), 'f16': (torch.float16, 2.0 ** -11, 1024.0),
          'f32': (torch.float32, 0.0, 1.0)}


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
    act = torch.randint(0, A, (B,), generator=g, dtype=torch.int32)
    act[0] = A - 1
    act[B - 1] = 0
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
    rew = torch.randn(B, generator=g)
    done = (torch.rand(B, generator=g) < 0.2).float()
    gam = torch.tensor([0.99 ** (1 + i % 3) for i in range(B)])
    for i, (r, d, gm) in enumerate([(1.0, 1.0, 0.99), (0.5, 0.0, 0.0)][:B]):
        rew[i], done[i], gam[i] = r, d, gm
    wts, zrow = None, None
    if wmode != 'none':
        wts = torch.rand(B, generator=g) + 0.5
        if wmode == 'zero':
            zrow = 10 if B > 10 else B - 1
            wts[zrow] = 0.0
    rows = torch.full((3, B, KD), PAD_IN)
    rows[:, :, :A] = x
    if dueling:
        rows[:, :, VO] = v
    return dict(B=B, A=A, dueling=dueling, huber=huber, delta=delta, tau=tau, alpha=alpha, clip=clip,
                rows=rows.float(), rew=rew.float(), done=done, gam=gam.float(), act=act,
                wts=None if wts is None else wts.float(), tie=tie, zrow=zrow)


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
def _ext(variant):
    from dist_dqn_amd.ops import _ext as loader
    return loader.load(required=True, variant=variant)


def _flts(c):
    return [float(c['alpha']), float(c['tau']), float(c['clip']), float(c['delta'])]


def _train(ext, c, act_t):
    B, A = c['B'], c['A']
    KD = _kd(c['dueling'])
    t = {k: c[k].to(DEV).contiguous() for k in ('rows', 'rew', 'done', 'gam', 'act')}
    wts = None if c['wts'] is None else c['wts'].to(DEV)
    dout = torch.full(((B + 8) * KD,), SENT, dtype=act_t, device=DEV)
    prio = torch.full((B + 8,), SENT, dtype=torch.float32, device=DEV)
    parts = torch.full((72,), SENT, dtype=torch.float32, device=DEV)
    io = [t['act'].data_ptr(), t['rew'].data_ptr(), t['done'].data_ptr(), t['gam'].data_ptr(),
          0 if wts is None else wts.data_ptr(), 0, prio.data_ptr()] + [0] * 6
    lg = [t['rows'][i].data_ptr() for i in range(3)]
    ext.qnet_mdqn_head([B, A, HID, int(c['dueling']), int(c['huber']), 0], [1], _flts(c), [], [], [], [], [], io,
                       [], [], [], [], [], lg, 0, [parts.data_ptr(), dout.data_ptr()])
    torch.cuda.synchronize()
    return dout.cpu(), prio.cpu(), parts.cpu()


_ratios = {}


def _check_train(variant, c):
    act_t, ulp, scale = BUILDS[variant]
    B, A = c['B'], c['A']
    KD = _kd(c['dueling'])
    ref = _reference(c)
    ext = _ext(variant)
    dout, prio, parts = _train(ext, c, act_t)
    dout2, prio2, parts2 = _train(ext, c, act_t)
    assert torch.equal(prio, prio2) and torch.equal(dout.view(torch.uint8), dout2.view(torch.uint8)) \
        and torch.equal(parts, parts2), 'repeatability'
    # layout and write coverage
    d = dout.double().view(B + 8, KD).numpy()
    g, cf, mask = _dout_ref(c, ref)
    assert (d[:B][:, ~mask] == SENT).all(), 'a pad column was written'
    assert (d[B:] == SENT).all() and (prio[B:] == SENT).all(), 'a row beyond B was written'
    assert (d[:B][:, mask] != SENT).all() and (prio[:B] != SENT).all(), 'a Q / value column was left unwritten'
    nb = _blocks(B)
    assert (parts[nb:] == SENT).all() and (parts[:nb] != SENT).all(), 'loss partials'
    assert np.isfinite(d[:B][:, mask]).all() and torch.isfinite(prio[:B]).all() and torch.isfinite(parts[:nb]).all()
    # priorities |d| and the loss (the fc dgrad launch's aux duty: sum / B)
    pk = prio[:B].double().numpy()
    print('prio: max |err| %.3g at |d| up to %.3g' % (np.abs(pk - ref['ad']).max(), ref['ad'].max()))
    np.testing.assert_allclose(pk, ref['ad'], rtol=1e-4, atol=1e-5)
    loss_ref = float((ref['w'] * ref['per']).sum() / B)
    np.testing.assert_allclose(float(parts[:nb].double().sum()) / B, loss_ref, rtol=1e-4, atol=1e-5)
    # dL/dQ rows: every written element of every row is compared (nothing is excluded)
    wb = (ref['w'] / B)[:, None]
    want = g * wb * scale
    bound = (ulp + 5 * E24) * np.abs(want) + _t_g(c, ref)[:, None] * cf * wb * scale
    err = np.abs(d[:B] - want)
    sel = np.broadcast_to(mask[None, :], err.shape)            # (no row mask: nothing is excluded)
    assert int(sel.sum()) == B * (A + int(c['dueling'])), 'every written element of every row is compared'
    ratio = np.where(sel & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    _ratios[variant] = max(_ratios.get(variant, 0.0), float(ratio.max()))
    print('dout16 %r: max err / bound %.3f (build so far %.3f)' % (variant, ratio.max(), _ratios[variant]))
    bad = sel & (err > bound)
    assert not bad.any(), (int(bad.sum()), [(int(b), int(k), d[b, k], want[b, k]) for b, k in np.argwhere(bad)[:5]])
    if c['zrow'] is not None:
        assert (d[c['zrow']][mask] == 0.0).all(), 'zero-weight row'
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
def _infer(ext, rows, B, A, dueling):
    r = rows.to(DEV).contiguous()
    q = torch.full((B * A + 8,), float('nan'), dtype=torch.float32, device=DEV)
    ext.qnet_mdqn_head([B, A, HID, int(dueling), 0, 1], [1], [0.9, 0.03, -1.0, 1.0], [], [], [], [], [],
                       [0] * 7 + [q.data_ptr()] + [0] * 5, [], [], [], [], [], [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    return q.cpu()


INFER_POINTS = [(2, 0), (4, 1), (5, 0), (8, 1), (9, 1), (16, 1), (17, 1), (18, 1), (19, 0), (32, 1), (32, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 32, 513])
@pytest.mark.parametrize('A,dueling', INFER_POINTS)
def test_mdqn_infer_matches_float64(A, dueling, B):
    """q_values' kernel: the dueling combine (B = 513: more rows than the block's 64 row groups
    take in eight passes)."""
    c = _inputs(B, A, dueling, 0, 1.0, 'none', 0.03, 0.9, _seed(B, A, dueling, 0))
    q = _infer(_ext(''), c['rows'][0], B, A, dueling)
    assert torch.isnan(q[B * A:]).all(), 'written beyond [B][A]'
    assert not torch.isnan(q[:B * A]).any(), 'q_out left unwritten'
    q64, mag = _q64(c['rows'][0], A, dueling)
    err = np.abs(q[:B * A].double().numpy().reshape(B, A) - q64)
    bound = (11 if dueling else 0) * E24 * mag[:, None]
    print('q: max err / (11 e M) %.3f' % (err / (11 * E24 * mag[:, None])).max())
    assert (err <= bound).all(), float((err / (11 * E24 * mag[:, None])).max())
