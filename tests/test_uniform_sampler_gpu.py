"""The uniform without-replacement sampler (`draw_distinct`, sample_dev.h) against its exact replica.

sample_dev.h promises "deterministic in (seed, ctr, n, B): every caller gets the same indices";
this pins what those indices are (tests/philox_ref.py replays the rejection rounds and the serial
bitmap fix-up with integer arithmetic only), and checks uniformity once more without the replica.

Measured on an MI355X: every index equal; chi-square over 64 bins = 63.62, threshold 131.74
(the replica on the CPU gives the same 63.62: same indices).
"""
import numpy as np
import pytest
import torch

import philox_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _sample(size, seed, ctr, B, launches=1, sample_out=None):
    from dist_dqn_amd.ops import kernels
    size_t = torch.tensor([size], dtype=torch.int32, device=DEV)
    rng = torch.tensor([seed, ctr], dtype=torch.int64, device=DEV)
    outs = []
    for _ in range(launches):
        out = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        kernels.replay_sample_uniform(size_t, rng, out, sample_out)
        outs.append(out)
    assert rng.cpu().tolist() == [seed, ctr + launches]           # the device advances the counter
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize('seed', R.UNIFORM_SEEDS)
@pytest.mark.parametrize('n,B', R.UNIFORM_CASES)
def test_uniform_sampler_equals_replica(n, B, seed):
    got = _sample(n, seed, 0, B, launches=R.UNIFORM_COUNTERS)
    for ctr, g in enumerate(got):
        want, _ = R.draw_distinct_ref(seed, ctr, n, B)
        assert np.array_equal(g, want), (ctr, np.flatnonzero(g != want)[:8])


def test_uniform_sampler_size_zero_is_one():
    (got,) = _sample(0, 123, 4, 8)
    want, _ = R.draw_distinct_ref(123, 4, 1, 8)
    assert np.array_equal(got, want) and (got == 0).all()


@pytest.mark.parametrize('n,B,K', [(10000, 32, 4), (100, 100, 1)])      # rejection only / serial fix-up
def test_uniform_sample_out_gathers_at_the_indices(n, B, K):
    t = np.arange(n)
    cols = dict(state_idx=(4 * t[:, None] + np.arange(K)[None, :]).astype(np.int32),
                next_idx=(100000 + t).astype(np.int32), actions=t.astype(np.int32),
                rewards=(t + 0.25).astype(np.float32), dones=(t % 2).astype(np.float32),
                gammas=(0.5 + t / 16384.0).astype(np.float32))
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in cols.items()}
    outs = [torch.full((B,), -1, dtype=torch.int32, device=DEV)] + \
           [torch.full((B,), float('nan'), device=DEV) for _ in range(3)] + \
           [torch.full((B, K), -1, dtype=torch.int32, device=DEV) for _ in range(2)]
    so = [dev[k] for k in ('state_idx', 'next_idx', 'actions', 'rewards', 'dones', 'gammas')] + outs
    (idx,) = _sample(n, 0, 0, B, sample_out=so)
    want, fixup = R.draw_distinct_ref(0, 0, n, B)
    assert fixup == (n == 100)
    assert np.array_equal(idx, want)
    a, r, d, g, st, nx = [o.cpu().numpy() for o in outs]
    assert np.array_equal(a, cols['actions'][idx]) and np.array_equal(r, cols['rewards'][idx])
    assert np.array_equal(d, cols['dones'][idx]) and np.array_equal(g, cols['gammas'][idx])
    assert np.array_equal(st, cols['state_idx'][idx])
    assert np.array_equal(nx, np.concatenate([cols['state_idx'][idx][:, 1:], cols['next_idx'][idx][:, None]], 1))


def test_uniform_sampler_chi_square():
    """Replica-free: n = 4096, B = 64, 400 launches, 64 bins of 64 indices; fails above the
    1 - 1e-6 quantile of chi2(63), 131.74 by Wilson-Hilferty (philox_ref.chi2_threshold)."""
    draws = _sample(R.CHI2_N, R.CHI2_SEED, 0, R.CHI2_B, launches=R.CHI2_LAUNCHES)
    for d in draws:
        assert d.min() >= 0 and d.max() < R.CHI2_N and len(set(d.tolist())) == R.CHI2_B
    chi2, thr = R.chi2_of(draws), R.chi2_threshold()
    print('uniform sampler chi2 = %.2f (threshold %.2f)' % (chi2, thr))
    assert chi2 < thr
