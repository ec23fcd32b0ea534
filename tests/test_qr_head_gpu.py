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

The inputs and the reference live in qr_ref.py (the wide head's tests use them too), the launches
and the assertions on their outputs in head_ref.py.
"""
import pytest
import torch

import qr_ref
from head_ref import DEV, HID, dims, ext

FN = 'qnet_qr_head'
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
INFER_POINTS = [(2, 51, 0), (4, 51, 1), (5, 51, 0), (8, 51, 1), (9, 51, 1), (18, 51, 1), (19, 51, 0),
                (6, 2, 1), (6, 21, 1), (4, 32, 1), (5, 32, 0), (6, 33, 1), (6, 64, 1), (18, 64, 0)]
_ratios = {}


def _blocks(B):
    return min((B + 7) // 8, 64)   # eight samples (one per wave) per learner block


def test_seeded_cases_stay_within_the_near_tie_cap():
    """No GPU: the reference alone, for every case this file launches."""
    qr_ref.check_near_tie_cap(TRAIN_CASES + [OTHER_BUILDS_CASE])


@pytest.mark.gpu
@pytest.mark.parametrize('B,A,N,dueling,double,wmode,kappa', TRAIN_CASES)
def test_qr_train_matches_float64(B, A, N, dueling, double, wmode, kappa):
    qr_ref.check_train('', (B, A, N, dueling, double, wmode, kappa), FN, _blocks(B), _ratios)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['f16', 'f32'])
def test_qr_train_other_builds(variant):
    qr_ref.check_train(variant, OTHER_BUILDS_CASE, FN, _blocks(OTHER_BUILDS_CASE[0]), _ratios)


@pytest.mark.gpu
def test_qr_head_refuses_bad_arguments():
    """Quantile count, kappa and the inference batch's LDS are checked before any launch."""
    r = torch.zeros(4, dims(6, 65, 0)[2], device=DEV)
    q = torch.full((2048 * 18,), float('nan'), dtype=torch.float32, device=DEV)
    io = [0] * 7 + [q.data_ptr()] + [0] * 5
    for n, kappa, B, A, word in ((65, 1.0, 4, 6, 'quantiles'), (1, 1.0, 4, 6, 'quantiles'), (51, 0.0, 4, 6, 'kappa'),
                                 (51, 1.0, 2048, 18, 'too large')):
        with pytest.raises(RuntimeError, match=word):
            ext('').qnet_qr_head([B, A, HID, 0, 0, 1], [n], [kappa], [], [], [], [], [], io, [], [], [], [], [],
                                 [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    assert torch.isnan(q).all()


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 32, 513])
@pytest.mark.parametrize('A,N,dueling', INFER_POINTS)
def test_qr_infer_matches_float64(A, N, dueling, B):
    """q_values' kernel: Q = mean over quantiles (B = 513 with 19 actions: more rows than the
    block's 64 row groups take in eight passes)."""
    qr_ref.check_infer(FN, B, A, N, dueling)
