"""The prioritized sampler (`per_sample_lane`, sumtree_dev.h) against its exact Philox replica.

Leaves must equal the replica bit for bit (tests/philox_ref.py: the same fp32 stratified draw, a
one-level-at-a-time walk); weights are compared with the float64 weights of the replica's leaves.
Trees cover every last-round depth of the 4-levels-per-round-trip descent (L = 0, 1, 3, 4, 5, 10,
12, 20) and are built with NumPy, not with the update kernel.

Weight bound: relative (4 beta + 1 + 2k) 2^-24 -- two roundings in each of n p and n p_min, scaled
by beta, two powf calls at k ulp each, one division. k = 16: the OpenCL full-profile bound for pow
that OCML is built to meet (the installed ROCm documentation carries no accuracy table).
Measured on an MI355X, max err / bound over all trees and batches:
beta = 0: 0 (every weight exactly 1); beta = 0.4: 0.099; beta = 1: 0.122. Leaves: 0 lanes differ.

A zero-priority leaf gives p_min = 0, so every weight of such a tree is 0 for beta > 0 (kernel and
replica alike): the configuration always has eps > 0, and the test pins that behaviour as it is.
"""
import numpy as np
import pytest
import torch

import philox_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
K_ULP = 16
_worst = {}


def _device_tree(capacity, pattern):
    from dist_dqn_amd.replay.sumtree import DeviceSumTree
    leaves, size = R.per_leaves(capacity, pattern)
    tree = DeviceSumTree(capacity, DEV)
    s32, m32 = R.build_tree(leaves, tree.P)
    tree.sum.copy_(torch.from_numpy(s32))
    tree.min.copy_(torch.from_numpy(m32))
    return tree, leaves, size, s32, m32


def _launch(tree, seed, ctr, size, B, beta, sample_out=None):
    from dist_dqn_amd.ops import kernels
    rng = torch.tensor([seed, ctr], dtype=torch.int64, device=DEV)
    idx = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    w = torch.full((B,), float('nan'), device=DEV)
    if not isinstance(beta, tuple):
        beta = torch.tensor([beta], dtype=torch.float32, device=DEV)
    kernels.sumtree_sample(tree, rng, torch.tensor([size], dtype=torch.int32, device=DEV), beta, idx, w, sample_out)
    return idx.cpu().numpy(), w.cpu().numpy(), rng.cpu().tolist()


@pytest.mark.parametrize('capacity,pattern', R.per_cases())
def test_per_sampler_equals_replica(capacity, pattern):
    tree, leaves, size, s32, m32 = _device_tree(capacity, pattern)
    P = tree.P
    for beta in R.PER_BETAS:
        b32 = np.float32(beta)
        bound = (4 * beta + 1 + 2 * K_ULP) * 2.0 ** -24
        for B in R.PER_BATCHES:
            # two consecutive launches, + the launch whose last lane sits on the tree total
            for ctr in [0, 1] + ([R.PER_EDGE_CTR] if B == R.PER_EDGE_B else []):
                idx, w, rng = _launch(tree, R.PER_SEED, ctr, size, B, float(b32))
                assert rng == [R.PER_SEED, ctr + 1]
                leaf, w_ref = R.per_sample_ref(s32, m32, R.PER_SEED, ctr, size, B, P, b32)
                assert np.array_equal(idx, leaf), (beta, B, ctr, np.flatnonzero(idx != leaf)[:8])
                if beta == 0:
                    assert (w == 1.0).all()
                err = np.abs(w.astype(np.float64) - w_ref)
                ratio = float((err / (bound * np.maximum(w_ref, 1e-300))).max()) if (w_ref > 0).any() else 0.0
                _worst[beta] = max(_worst.get(beta, 0.0), ratio)
                assert (err <= bound * w_ref).all(), (beta, B, ctr, ratio)
                # max-normalised: no weight above 1, and the minimum-priority leaf has weight 1
                if m32[1] > 0:
                    assert w.max() <= 1.0 + bound
                    if (s32[P + leaf] == m32[1]).any():
                        assert abs(float(w.max()) - 1.0) <= bound
    print('per weights, max err / bound so far:', {b: round(v, 4) for b, v in sorted(_worst.items())})
    # a sample launch only reads the trees
    assert np.array_equal(tree.sum.cpu().numpy(), s32) and np.array_equal(tree.min.cpu().numpy(), m32)


@pytest.mark.parametrize('step', [0, 250, 1000, 5000])
def test_per_beta_schedule_equals_float_beta(step):
    """An int64 step anneals beta = min(1, beta0 + (1 - beta0) step / steps) in the kernel: bit for
    bit the float-beta launch with that expression evaluated in fp32, from the same RNG state."""
    tree, _, size, s32, m32 = _device_tree(1000, 'loguniform')
    b0, steps = np.float32(0.4), np.float32(1000)
    beta = min(np.float32(1), b0 + (np.float32(1) - b0) * np.float32(step) / steps)
    assert isinstance(beta, np.float32)
    assert beta == (b0 if step == 0 else 1 if step >= 1000 else beta) and b0 <= beta <= 1
    for B in (64, 100):
        st = torch.tensor([step], dtype=torch.int64, device=DEV)
        i1, w1, r1 = _launch(tree, 11, 5, size, B, (st, 0.4, 1000))
        i2, w2, r2 = _launch(tree, 11, 5, size, B, float(beta))
        assert r1 == r2 == [11, 6] and int(st.item()) == step
        assert np.array_equal(i1, i2)
        assert np.array_equal(w1.view(np.uint32), w2.view(np.uint32)), (step, B)
        if 0 < step < 1000:                         # the schedule really moved: not the beta0 weights
            _, w0, _ = _launch(tree, 11, 5, size, B, float(b0))
            assert not np.array_equal(w0, w1)


@pytest.mark.parametrize('K', [1, 4])
@pytest.mark.parametrize('pattern', ['loguniform', 'partial'])
def test_per_sample_out_gathers_at_the_leaves(K, pattern):
    C, B = 1000, 100
    tree, _, size, s32, m32 = _device_tree(C, pattern)
    t = np.arange(C)
    cols = dict(state_idx=(4 * t[:, None] + np.arange(K)[None, :]).astype(np.int32),
                next_idx=(100000 + t).astype(np.int32), actions=t.astype(np.int32),
                rewards=(t + 0.25).astype(np.float32), dones=(t % 2).astype(np.float32),
                gammas=(0.5 + t / 4096.0).astype(np.float32))
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in cols.items()}
    outs = [torch.full((B,), -1, dtype=torch.int32, device=DEV)] + \
           [torch.full((B,), float('nan'), device=DEV) for _ in range(3)] + \
           [torch.full((B, K), -1, dtype=torch.int32, device=DEV) for _ in range(2)]
    so = [dev[k] for k in ('state_idx', 'next_idx', 'actions', 'rewards', 'dones', 'gammas')] + outs
    idx, _, _ = _launch(tree, 3, 0, size, B, 0.4, so)
    leaf, _ = R.per_sample_ref(s32, m32, 3, 0, size, B, tree.P, np.float32(0.4))
    assert np.array_equal(idx, leaf)
    a, r, d, g, st, nx = [o.cpu().numpy() for o in outs]
    assert np.array_equal(a, cols['actions'][leaf]) and np.array_equal(r, cols['rewards'][leaf])
    assert np.array_equal(d, cols['dones'][leaf]) and np.array_equal(g, cols['gammas'][leaf])
    assert np.array_equal(st, cols['state_idx'][leaf])
    assert np.array_equal(nx, np.concatenate([cols['state_idx'][leaf][:, 1:], cols['next_idx'][leaf][:, None]], 1))
    for k, v in cols.items():                       # the replay columns are only read
        assert np.array_equal(dev[k].cpu().numpy(), v)
