"""The QR-DQN head kernels (csrc/kernels/qr_head.hip: qr_train_kernel, qr_infer_kernel) against a
float64 reference of the same operation, at the shapes where the kernels change path.

As in test_c51_head_gpu.py the binding takes the output rows as pointers, so the kernels run on
synthetic fp32 rows with no network: ``KD`` floats = [A * N quantiles | pad | dueling value
quantiles at VO | pad] (VO = A * N rounded up to 32). The input pads hold 1e9 (a kernel that read
one would show it) and the outputs start as a sentinel (a written pad column would show).

Reference (numpy float64, on the fp32 input values; nothing from ``models/losses.py``): dueling
combine per quantile, Q = mean over quantiles, argmax of the selection instance (first maximum
wins, an explicit loop), T_j = r + gamma (1 - done) theta_target(a*)_j, u_ij = T_j - theta(a)_i,
rho_ij = |tau_i - 1{u_ij < 0}| L_kappa(u_ij) / kappa, per = sum_i 1/N sum_j rho_ij and
g_i = -1/N sum_j |tau_i - 1{u_ij < 0}| clamp(u_ij, -kappa, kappa) / kappa; dL/dtheta = w / B g
(dueling: advantage columns times (i == a) - 1 / A, value columns plain).

Cases: action counts on both sides of every template instance (AM = 4, 8, 18, 32); N = 2, 21,
32 (VO == NO), 33, 51, 64; B = 1, 8, 9, 24 and 513 (the block-stride loop); plain / dueling, with
and without the Double-DQN instance; weights absent, random, containing an exact 0; kappa 1 and
0.5. Row 0 is terminal, row 1 has gamma = 0, a fifth of the rest are terminal; row 8 is scaled
by 30; row 9 (Double DQN cases) has two actions with bit-identical selection rows, the greedy ones.

Bounds. ``prio`` and the loss: rtol 1e-4, atol 1e-5 (the C51 head test's bound for a per-sample
fp32 reduction). ``dout16`` elementwise: |err| <= ulp |ref| + t, ulp = 2^-8 (bf16), 2^-11 (fp16),
0 (fp32) the storage step, and t = t_g |coef| w_b / B times the fp16 build's loss scale, with
coef the dueling coefficient and t_g the fp32 error of g_i, derived with e = 2^-24:
  * u_ij. theta_i and the target quantile each come out of the dueling combine (A - 1 adds for
    the action mean, its scaling, v - mean, x + v: A + 2 roundings of values up to M, twice),
    T_j is one fused multiply-add, u one subtraction: |du| <= (2 (A + 2) + 2) e M with dueling,
    2 e M without, M = the row's largest |input|, |T_j| or |theta_i|;
  * one term |tau_i - 1{u < 0}| clamp(u, -kappa, kappa) / kappa moves by at most |du| / kappa:
    unclipped it is linear in u with weight <= 1; clipped it does not move; at the knee and at
    the indicator flip (where |u| <= |du|) the term is continuous, so the same bound holds;
    the mean over j keeps it: |du| / kappa;
  * the N-term sum of terms <= 1: N adds, each rounding a partial sum <= N, over N: N e; the
    tau / weight products and the final scaling: 4 e more (|g| <= 1).
  t_g = ((2 (A + 2) + 2) or 2) e M / kappa + (N + 4) e.
A row whose two largest selection Q values lie within 1e-4 of the row's quantile range (largest
minus smallest selection quantile) in the reference is left out (fp32 cannot be asked to pick
float64's action there; the exact tie is not such a row); at most one row in 16, asserted per
case on the reference alone and, for every seeded case, in a test that needs no GPU. The loss
reference takes the kernel's own priority for such a row. The indicator flip and the Huber knee
need no exclusion (see above).

Q of the inference kernel, per row with M its largest |input|: an N-term mean of values <= M
is within N e M; plain heads add the scaling: (N + 2) e M; dueling combines three such means
(the action's, the value's, and the action mean of A of them: A e M more) in four more
operations: (3 N + A + 4) e M.

Largest observed err / bound over all cases of the build (one MI355X run): bf16 0.992 and fp16
0.960 (the storage rounding: round-to-nearest reaches the full step at the bottom of a binade),
fp32 0.087; Q of the inference kernel 0.138. Largest |err| of ``prio`` 1.7e-4 at values up to 1.4e3.
"""
import numpy as np
import pytest
import torch

DEV = torch.device('cuda', 0)
SENT = -4096.0                 # exact in bf16 / fp16 / fp32, below anything the kernels can write
PAD_IN = 1e9
HID = 128                      # (unused by the QR kernels; the binding wants a multiple of 128)
E24 = 2.0 ** -24
# variant -> (act_t as HipExecutor.act_dtype maps it, storage rounding step, kLossScale)
BUILDS = {'': (torch.bfloat16, 2.0 ** -8, 1.0), 'f16': (torch.float16, 2.0 ** -11, 1024.0),
          'f32': (torch.float32, 0.0, 1.0)}


def _dims(A, N, dueling):
    NO = A * N
    VO = (NO + 31) // 32 * 32
    return NO, VO, VO + ((N + 31) // 32 * 32 if dueling else 0)


def _blocks(B):
    return min((B + 7) // 8, 64)


# ------------------------------------------------------------------ inputs (CPU, seeded)
def _inputs(B, A, N, dueling, double, wmode, kappa, seed):
    g = torch.Generator().manual_seed(seed)
    NO, VO, KD = _dims(A, N, dueling)
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
    rew = torch.randn(B, generator=g)
    done = (torch.rand(B, generator=g) < 0.2).float()
    gam = torch.tensor([0.99 ** (1 + i % 3) for i in range(B)])
    for i, (r, d, gm) in enumerate([(1.0, 1.0, 0.99), (0.5, 0.0, 0.0)][:B]):
        rew[i], done[i], gam[i] = r, d, gm
    act = torch.randint(0, A, (B,), generator=g, dtype=torch.int32)
    act[0] = A - 1
    act[B - 1] = 0
    wts, zrow = None, None
    if wmode != 'none':
        wts = torch.rand(B, generator=g) + 0.5
        if wmode == 'zero':
            zrow = 10 if B > 10 else B - 1
            wts[zrow] = 0.0
    rows = torch.full((3, B, KD), PAD_IN)
    rows[:, :, :NO] = x.reshape(3, B, NO)
    if dueling:
        rows[:, :, VO:VO + N] = v
    return dict(B=B, A=A, N=N, dueling=dueling, double=double, kappa=kappa, rows=rows.float(), rew=rew.float(),
                done=done, gam=gam.float(), act=act, wts=None if wts is None else wts.float(), tie=tie, zrow=zrow)


# ------------------------------------------------------------------ float64 reference
def _quantiles64(rows, A, N, dueling):
    """Quantiles [.., A, N] (dueling combined) of output rows [.., KD], and the largest |input| [..]."""
    NO, VO, _ = _dims(A, N, dueling)
    r = rows.double().numpy()
    x = r[..., :NO].reshape(r.shape[:-1] + (A, N))
    mag = np.abs(r[..., :NO]).max(-1)
    if dueling:
        mag = np.maximum(mag, np.abs(r[..., VO:VO + N]).max(-1))
        x = x + r[..., None, VO:VO + N] - x.mean(-2, keepdims=True)
    return x, mag


def _reference(c):
    B, A, N, k = c['B'], c['A'], c['N'], float(c['kappa'])
    th, mag = _quantiles64(c['rows'], A, N, c['dueling'])     # [3, B, A, N], [3, B]
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


def _dout_ref(c, ref):
    """(g [B, KD] before the w / B factor, |dueling coefficient| [B, KD], written-column mask [KD])."""
    B, A, N = c['B'], c['A'], c['N']
    NO, VO, KD = _dims(A, N, c['dueling'])
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


def _t_g(c, ref):
    """fp32 error bound of g_i per row (see the module docstring)."""
    du = (2 * (c['A'] + 2) + 2 if c['dueling'] else 2) * E24 * ref['M']
    return du / float(c['kappa']) + (c['N'] + 4) * E24


# ------------------------------------------------------------------ launches
def _ext(variant):
    from dist_dqn_amd.ops import _ext as loader
    return loader.load(required=True, variant=variant)


def _train(ext, c, act_t):
    B, A, N = c['B'], c['A'], c['N']
    _, _, KD = _dims(A, N, c['dueling'])
    t = {k: c[k].to(DEV).contiguous() for k in ('rows', 'rew', 'done', 'gam', 'act')}
    wts = None if c['wts'] is None else c['wts'].to(DEV)
    dout = torch.full(((B + 8) * KD,), SENT, dtype=act_t, device=DEV)
    prio = torch.full((B + 8,), SENT, dtype=torch.float32, device=DEV)
    parts = torch.full((72,), SENT, dtype=torch.float32, device=DEV)
    io = [t['act'].data_ptr(), t['rew'].data_ptr(), t['done'].data_ptr(), t['gam'].data_ptr(),
          0 if wts is None else wts.data_ptr(), 0, prio.data_ptr()] + [0] * 6
    lg = [t['rows'][i].data_ptr() for i in range(3 if c['double'] else 2)]
    ext.qnet_qr_head([B, A, HID, int(c['dueling']), 0, 0], [N], [float(c['kappa'])], [], [], [], [], [], io,
                     [], [], [], [], [], lg, 0, [parts.data_ptr(), dout.data_ptr()])
    torch.cuda.synchronize()
    return dout.cpu(), prio.cpu(), parts.cpu()


_ratios = {}


def _check_train(variant, c):
    act_t, ulp, scale = BUILDS[variant]
    B, A, N = c['B'], c['A'], c['N']
    NO, VO, KD = _dims(A, N, c['dueling'])
    ref = _reference(c)
    skip = ref['skip']
    assert int(skip.sum()) * 16 <= B, ('near-ties in the reference: pick another seed', np.nonzero(skip)[0])
    keep = ~skip
    ext = _ext(variant)
    dout, prio, parts = _train(ext, c, act_t)
    dout2, prio2, _ = _train(ext, c, act_t)
    assert torch.equal(prio, prio2) and torch.equal(dout.view(torch.uint8), dout2.view(torch.uint8)), 'repeatability'
    # layout and write coverage
    d = dout.double().view(B + 8, KD).numpy()
    g, cf, mask = _dout_ref(c, ref)
    assert (d[:B][:, ~mask] == SENT).all(), 'a pad column was written'
    assert (d[B:] == SENT).all() and (prio[B:] == SENT).all(), 'a row beyond B was written'
    assert (d[:B][:, mask] != SENT).all() and (prio[:B] != SENT).all(), 'a quantile / value column was left unwritten'
    nb = _blocks(B)
    assert (parts[nb:] == SENT).all() and (parts[:nb] != SENT).all(), 'loss partials'
    # priorities (the unweighted per-sample loss) and the loss (the fc dgrad launch's aux duty: sum / B)
    pk = prio[:B].double().numpy()
    print('per: max |err| %.3g at |per| up to %.3g' % (np.abs(pk - ref['per'])[keep].max(), ref['per'].max()))
    np.testing.assert_allclose(pk[keep], ref['per'][keep], rtol=1e-4, atol=1e-5)
    loss_ref = float((ref['w'] * np.where(keep, ref['per'], pk)).sum() / B)
    np.testing.assert_allclose(float(parts[:nb].double().sum()) / B, loss_ref, rtol=1e-4, atol=1e-5)
    # dL/dtheta rows
    wb = (ref['w'] / B)[:, None]
    want = g * wb * scale
    bound = ulp * np.abs(want) + _t_g(c, ref)[:, None] * cf * wb * scale
    err = np.abs(d[:B] - want)
    sel = keep[:, None] & mask[None, :]
    ratio = np.where(sel & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    _ratios[variant] = max(_ratios.get(variant, 0.0), float(ratio.max()))
    print('dout16 %r: max err / bound %.3f (build so far %.3f)' % (variant, ratio.max(), _ratios[variant]))
    bad = sel & (err > bound)
    assert not bad.any(), (int(bad.sum()), [(int(b), int(k), d[b, k], want[b, k]) for b, k in np.argwhere(bad)[:5]])
    if c['zrow'] is not None:
        assert (d[c['zrow']][mask] == 0.0).all(), 'zero-weight row'


TRAIN_CASES = [
    # B, A, N, dueling, double, weights, kappa
    (24, 2, 51, 0, 0, 'none', 1.0), (24, 4, 51, 1, 1, 'rand', 1.0), (24, 5, 51, 0, 1, 'zero', 0.5),
    (24, 8, 51, 1, 0, 'rand', 1.0), (24, 9, 51, 1, 1, 'none', 0.5), (24, 18, 51, 1, 1, 'zero', 1.0),
    (24, 19, 51, 0, 1, 'rand', 1.0),                                               # AM boundaries
    (24, 6, 2, 1, 1, 'rand', 1.0), (24, 6, 21, 1, 0, 'none', 0.5),                 # under one 32-column tile
    (24, 4, 32, 1, 1, 'rand', 1.0), (24, 5, 32, 0, 0, 'zero', 1.0), (24, 18, 32, 1, 1, 'none', 1.0),   # VO == NO
    (24, 6, 33, 1, 1, 'rand', 0.5), (24, 6, 64, 1, 1, 'zero', 1.0), (24, 19, 64, 0, 0, 'rand', 1.0),
    (1, 6, 51, 1, 1, 'zero', 1.0), (8, 6, 51, 0, 1, 'rand', 1.0), (9, 6, 51, 1, 0, 'none', 1.0),
    (513, 6, 51, 1, 1, 'zero', 1.0),                                               # the block-stride loop
]
OTHER_BUILDS_CASE = (24, 6, 51, 1, 1, 'zero', 1.0)


def _seed(B, A, N, dueling, double):
    return 1000 * A + 10 * N + B + 2 * dueling + double


def _make(case):
    B, A, N, dueling, double, wmode, kappa = case
    return _inputs(B, A, N, dueling, double, wmode, kappa, _seed(B, A, N, dueling, double))


def test_seeded_cases_stay_within_the_near_tie_cap():
    """No GPU: the reference alone, for every case this file launches."""
    for case in TRAIN_CASES + [OTHER_BUILDS_CASE]:
        c = _make(case)
        ref = _reference(c)
        assert int(ref['skip'].sum()) * 16 <= c['B'], (case, np.nonzero(ref['skip'])[0])
        assert c['tie'] is None or not ref['skip'][c['tie'][0]]
        assert (ref['per'] >= 0).all() and (np.abs(ref['g']) <= 1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('B,A,N,dueling,double,wmode,kappa', TRAIN_CASES)
def test_qr_train_matches_float64(B, A, N, dueling, double, wmode, kappa):
    _check_train('', _make((B, A, N, dueling, double, wmode, kappa)))


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['f16', 'f32'])
def test_qr_train_other_builds(variant):
    _check_train(variant, _make(OTHER_BUILDS_CASE))


@pytest.mark.gpu
def test_qr_head_refuses_bad_arguments():
    """Quantile count, kappa and the inference batch's LDS are checked before any launch."""
    ext = _ext('')
    r = torch.zeros(4, _dims(6, 65, 0)[2], device=DEV)
    q = torch.full((2048 * 18,), float('nan'), dtype=torch.float32, device=DEV)
    io = [0] * 7 + [q.data_ptr()] + [0] * 5
    for n, kappa, B, A, word in ((65, 1.0, 4, 6, 'quantiles'), (1, 1.0, 4, 6, 'quantiles'), (51, 0.0, 4, 6, 'kappa'),
                                 (51, 1.0, 2048, 18, 'too large')):
        with pytest.raises(RuntimeError, match=word):
            ext.qnet_qr_head([B, A, HID, 0, 0, 1], [n], [kappa], [], [], [], [], [], io, [], [], [], [], [],
                             [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    assert torch.isnan(q).all()


# ------------------------------------------------------------------ inference kernel
def _infer(ext, rows, B, A, N, dueling):
    r = rows.to(DEV).contiguous()
    q = torch.full((B * A + 8,), float('nan'), dtype=torch.float32, device=DEV)
    ext.qnet_qr_head([B, A, HID, int(dueling), 0, 1], [N], [1.0], [], [], [], [], [],
                     [0] * 7 + [q.data_ptr()] + [0] * 5, [], [], [], [], [], [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    return q.cpu()


INFER_POINTS = [(2, 51, 0), (4, 51, 1), (5, 51, 0), (8, 51, 1), (9, 51, 1), (18, 51, 1), (19, 51, 0),
                (6, 2, 1), (6, 21, 1), (4, 32, 1), (5, 32, 0), (6, 33, 1), (6, 64, 1), (18, 64, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 32, 513])
@pytest.mark.parametrize('A,N,dueling', INFER_POINTS)
def test_qr_infer_matches_float64(A, N, dueling, B):
    """q_values' kernel: Q = mean over quantiles (B = 513 with 19 actions: more rows than the
    block's 64 row groups take in eight passes)."""
    c = _inputs(B, A, N, dueling, False, 'none', 1.0, _seed(B, A, N, dueling, 0))
    q = _infer(_ext(''), c['rows'][0], B, A, N, dueling)
    assert torch.isnan(q[B * A:]).all(), 'written beyond [B][A]'
    assert not torch.isnan(q[:B * A]).any(), 'q_out left unwritten'
    th, mag = _quantiles64(c['rows'][0], A, N, dueling)
    err = np.abs(q[:B * A].double().numpy().reshape(B, A) - th.mean(-1))
    bound = ((3 * N + A + 4) if dueling else (N + 2)) * E24 * mag[:, None]
    print('q: max err / bound %.3f' % (err / bound).max())
    assert (err <= bound).all(), float((err / bound).max())
