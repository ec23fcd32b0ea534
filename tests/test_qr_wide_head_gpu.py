"""The wide QR-DQN head kernels (csrc/kernels/qr_wide_head.hip: qr_wide_train_kernel,
qr_wide_infer_kernel; 64 < N <= 256 quantiles, N % 4 == 0) against a float64 reference of the same
operation, at the shapes where the kernels change path.

The method, the inputs, the reference and the bounds are those of test_qr_head_gpu.py (both
files take them from qr_ref.py and head_ref.py): synthetic fp32 rows ``KD`` = [A * N quantiles | pad | dueling value
quantiles at VO | pad] with 1e9 in the input pads, sentinel-filled outputs, a numpy float64
reference, two launches bit-equal, no pad column and no row beyond ``B`` written, every real
column written.

Cases: N = 68 and 72 (the smallest wide counts: two waves, the second with 4 / 8 threads and a
partial last lane group of the 16-byte loads), 128 / 132 (two full waves / a third wave of four
threads), 200 (the paper's count: four waves, the last with 8 threads), 252 / 256 (the last lane
of the streaming layout partial / every lane and thread in use); action counts at, just above
and well above the wave count (A = 2 on two waves; 4, 5, 6; 18 / 19 and 32: more than one
four-action load batch per wave); B = 1, 8, 9, 24, 32 and, more samples than the 64 learner blocks take at
once, 130 and 513; plain / dueling, with and without the Double-DQN instance; weights absent,
random, containing an exact 0; kappa 1 and 0.5.

Bounds (test_qr_head_gpu.py's docstring derives them). ``prio`` and the loss: rtol 1e-4, atol
1e-5. ``dout16`` elementwise: |err| <= ulp |ref| + t_g |coef| w_b / B times the fp16 build's loss
scale, t_g = ((2 (A + 2) + 2) or 2) e M / kappa + (N + 4) e: the (N + 4) e term holds for any
order of an N-term sum of terms <= 1, so the four accumulator chains of the pairwise loop and the
per-wave partials of the dueling action mean stay inside it. Near-tie rows are left out, at most
one row in 16, asserted per case on the reference alone and in a test that needs no GPU.
Q of the inference kernel: (3 N + A + 4) e M with dueling, (N + 2) e M plain.

Largest observed err / bound over all cases of the build (one MI355X run): bf16 0.993 and fp16
0.938 (the storage rounding reaches its full step at the bottom of a binade), fp32 0.042; Q of the
inference kernel 0.004. Largest |err| of ``prio`` seen 1.7e-4 at values up to 3.1e3.
"""
import pytest
import torch

import qr_ref
from head_ref import DEV, HID, dims, ext

FN = 'qnet_qr_wide_head'
TRAIN_CASES = [
    # B, A, N, dueling, double, weights, kappa
    (24, 2, 68, 0, 0, 'none', 1.0), (24, 6, 68, 1, 1, 'rand', 1.0), (24, 6, 72, 1, 0, 'zero', 0.5),
    (24, 4, 128, 1, 1, 'rand', 1.0), (24, 5, 128, 0, 1, 'zero', 1.0), (24, 6, 132, 1, 1, 'none', 0.5),
    (24, 6, 200, 1, 1, 'zero', 1.0), (32, 18, 200, 1, 1, 'rand', 1.0), (24, 19, 200, 0, 1, 'none', 1.0),
    (24, 32, 200, 1, 0, 'rand', 0.5),
    (24, 6, 252, 1, 1, 'rand', 1.0), (24, 6, 256, 1, 1, 'zero', 1.0), (24, 18, 256, 0, 0, 'rand', 1.0),
    (1, 6, 200, 1, 1, 'zero', 1.0), (8, 6, 200, 0, 1, 'rand', 1.0), (9, 6, 200, 1, 0, 'none', 1.0),
    (513, 6, 68, 1, 1, 'zero', 1.0), (130, 6, 200, 1, 1, 'rand', 1.0),      # more samples than learner blocks
]
OTHER_BUILDS_CASE = (24, 6, 200, 1, 1, 'zero', 1.0)
INFER_POINTS = [(2, 68, 0), (6, 72, 1), (5, 128, 0), (18, 200, 1), (19, 200, 0), (6, 252, 1), (18, 256, 0)]
_ratios = {}


def _blocks(B):
    return min(B, 64)              # one sample per learner block at a time


def test_seeded_cases_stay_within_the_near_tie_cap():
    """No GPU: the reference alone, for every case this file launches."""
    qr_ref.check_near_tie_cap(TRAIN_CASES + [OTHER_BUILDS_CASE])


@pytest.mark.gpu
@pytest.mark.parametrize('B,A,N,dueling,double,wmode,kappa', TRAIN_CASES)
def test_qr_wide_train_matches_float64(B, A, N, dueling, double, wmode, kappa):
    qr_ref.check_train('', (B, A, N, dueling, double, wmode, kappa), FN, _blocks(B), _ratios)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['f16', 'f32'])
def test_qr_wide_train_other_builds(variant):
    qr_ref.check_train(variant, OTHER_BUILDS_CASE, FN, _blocks(OTHER_BUILDS_CASE[0]), _ratios)


@pytest.mark.gpu
def test_qr_wide_head_refuses_bad_arguments():
    """Quantile count and kappa are checked before any launch: the output buffer stays untouched."""
    r = torch.zeros(4, dims(6, 260, 0)[2], device=DEV)
    q = torch.full((4 * 6,), float('nan'), dtype=torch.float32, device=DEV)
    io = [0] * 7 + [q.data_ptr()] + [0] * 5
    for n, kappa, word in ((64, 1.0, 'quantiles'), (66, 1.0, 'quantiles'), (260, 1.0, 'quantiles'), (200, 0.0, 'kappa')):
        with pytest.raises(RuntimeError, match=word):
            ext('').qnet_qr_wide_head([4, 6, HID, 0, 0, 1], [n], [kappa], [], [], [], [], [], io, [], [], [], [], [],
                                      [r.data_ptr()], 0, [])
    torch.cuda.synchronize()
    assert torch.isnan(q).all()


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 32, 513])
@pytest.mark.parametrize('A,N,dueling', INFER_POINTS)
def test_qr_wide_infer_matches_float64(A, N, dueling, B):
    """q_values' kernel: Q = mean over quantiles."""
    qr_ref.check_infer(FN, B, A, N, dueling)
