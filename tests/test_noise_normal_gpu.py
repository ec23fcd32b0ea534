"""The noisy-net normals (`noise_normal_kernel` / `noise_normals4`, common.h) against a float64
Box-Muller over the same Philox uniforms (tests/philox_ref.py).

Element-wise bound: 2^-9 max(1, |z|). The kernel uses `__logf` / `__sincosf`, so no ulp-level
claim is made; the bound is what the consumer needs (the normals go through
f(x) = sgn(x) sqrt|x| into bf16 weights, whose relative step is 2^-8), and an error in the index
mapping 4q + 2h + j over [out0 | out1] shows up as differences of order 1.
Measured on an MI355X: largest |err| / bound = 0.0007.
"""
import numpy as np
import pytest
import torch

import philox_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 64
_worst = [0.0]


def _ext():
    from dist_dqn_amd.ops import _ext
    return _ext.load(required=True)


def _launch(seed, ctr, n, two):
    """One launch into NaN-filled buffers with guard floats on both sides: (out0, out1, buffers, rng)."""
    bufs = [torch.full((n + 2 * GUARD,), float('nan'), device=DEV) for _ in range(2 if two else 1)]
    views = [b[GUARD:GUARD + n] for b in bufs]
    rng = torch.tensor([seed, ctr], dtype=torch.int64, device=DEV)
    _ext().noise_normal(views[0], views[1] if two else None, rng)
    return [b.cpu().numpy() for b in bufs], rng.cpu().tolist()


@pytest.mark.parametrize('two', [False, True])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 512, 513, 4099])
def test_noise_normal_equals_replica(n, two):
    seed, ctr = 5, 9
    bufs, rng = _launch(seed, ctr, n, two)
    assert rng == [seed, ctr + 1]
    refs = R.noise_normals_ref(seed, ctr, n, two)
    for buf, ref in zip(bufs, refs):
        # nothing outside [0, n) is touched, every element inside is written
        assert np.isnan(buf[:GUARD]).all() and np.isnan(buf[GUARD + n:]).all()
        z = buf[GUARD:GUARD + n].astype(np.float64)
        assert np.isfinite(z).all()
        ratio = np.abs(z - ref) / (2.0 ** -9 * np.maximum(1.0, np.abs(ref)))
        _worst[0] = max(_worst[0], float(ratio.max()))
        assert (ratio <= 1.0).all(), (np.flatnonzero(ratio > 1)[:8], float(ratio.max()))
    print('noise normals, max |err| / bound so far: %.5f' % _worst[0])


def test_noise_normal_moments():
    n = 2 ** 15                                             # 2^16 values over the two outputs
    (b0, b1), _ = _launch(5, 0, n, True)
    z0, z1 = b0[GUARD:GUARD + n].astype(np.float64), b1[GUARD:GUARD + n].astype(np.float64)
    z = np.concatenate([z0, z1])
    assert abs(z.mean()) < 5 / np.sqrt(z.size)
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)
    assert abs(np.corrcoef(z0, z1)[0, 1]) < 5 / np.sqrt(z.size)


def test_noise_normal_streams():
    """Consecutive launches draw fresh values; equal (seed, counter) draws equal values."""
    n = 513
    out0, out1 = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    rng = torch.tensor([5, 0], dtype=torch.int64, device=DEV)
    _ext().noise_normal(out0, out1, rng)
    first = torch.cat([out0, out1]).cpu().numpy()
    _ext().noise_normal(out0, out1, rng)
    second = torch.cat([out0, out1]).cpu().numpy()
    assert rng.cpu().tolist() == [5, 2]
    assert (first != second).mean() > 0.99
    for seed, ctr, same in [(5, 0, True), (5, 1, False), (6, 0, False)]:
        rng = torch.tensor([seed, ctr], dtype=torch.int64, device=DEV)
        _ext().noise_normal(out0, out1, rng)
        again = torch.cat([out0, out1]).cpu().numpy()
        assert np.array_equal(again, first) == same
    # the one-output launch draws the first n elements of the same stream
    rng = torch.tensor([5, 0], dtype=torch.int64, device=DEV)
    _ext().noise_normal(out0, None, rng)
    assert np.array_equal(out0.cpu().numpy(), first[:n])
