"""The NumPy replicas of the device samplers (tests/philox_ref.py), checked without a GPU:
known-answer vectors for the generator, the tree walk against the CPU fallback the project
already trusts, an independent float64 stratum check, and that the cases of the GPU tests reach
the code paths they are meant to reach."""
import numpy as np
import pytest
import torch

import philox_ref as R


def _tree(capacity, pattern):
    leaves, size = R.per_leaves(capacity, pattern)
    P = R.tree_P(capacity)
    s32, m32 = R.build_tree(leaves, P)
    return leaves, size, P, s32, m32


def _launches(B):
    return [0, 1] + ([R.PER_EDGE_CTR] if B == R.PER_EDGE_B else [])


# Random123 known-answer vectors of philox4x32-10: counter words c0..c3, key words k0 k1, output
KAT = [
    ([0x00000000] * 4, [0x00000000] * 2, [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize('c,k,want', KAT)
def test_philox_known_answers(c, k, want):
    got = R.philox(k[0] | (k[1] << 32), c[2] | (c[3] << 32), c[0], c[1])
    assert [int(v) for v in got] == want
    # vectorised over lo0 / lo1: the same words at every position of an array call
    lo0 = np.array([c[0], 5, c[0]], dtype=np.uint64)
    lo1 = np.array([c[1], c[1], c[1]], dtype=np.uint64)
    vec = R.philox(k[0] | (k[1] << 32), c[2] | (c[3] << 32), lo0, lo1)
    assert [int(v[0]) for v in vec] == want and [int(v[2]) for v in vec] == want
    assert [int(v[1]) for v in vec] != want


def test_u01_range_and_exactness():
    x = np.array([0, 255, 256, 0xffffffff], dtype=np.uint64)
    u = R.u01(x)
    assert u.dtype == np.float32
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]


def test_build_tree_is_consistent():
    leaves = np.array([0.5, 0.0, 3.0, 1e-3, 7.0], dtype=np.float32)
    s, m = R.build_tree(leaves, 8)
    assert s[8:13].tolist() == leaves.tolist() and s[13:].tolist() == [0.0] * 3
    assert m[8:13].tolist() == leaves.tolist() and np.isinf(m[13:]).all()
    for node in range(1, 8):
        assert s[node] == np.float32(s[2 * node] + s[2 * node + 1])
        assert m[node] == min(m[2 * node], m[2 * node + 1])
    assert m[1] == 0.0
    s1, m1 = R.build_tree(np.array([2.5], dtype=np.float32), 1)            # P = 1: the root is the leaf
    assert s1.tolist() == [0.0, 2.5] and m1[1] == 2.5


@pytest.mark.parametrize('capacity,pattern', R.per_cases())
def test_per_replica_walk_equals_cpu_fallback(capacity, pattern):
    """Fed the fallback's own torch.rand uniforms, the replica returns exactly the leaves of
    kernels.sumtree_sample on CPU tensors (a one-level-at-a-time walk the project trusts)."""
    from dist_dqn_amd.ops import kernels
    from dist_dqn_amd.replay.sumtree import DeviceSumTree
    _, size, P, s32, m32 = _tree(capacity, pattern)
    tree = DeviceSumTree(capacity, 'cpu')
    assert tree.P == P
    tree.sum.copy_(torch.from_numpy(s32))
    tree.min.copy_(torch.from_numpy(m32))
    for B in R.PER_BATCHES:
        for ctr in _launches(B):
            rng = torch.tensor([R.PER_SEED, ctr], dtype=torch.int64)
            uu = torch.rand(B, generator=kernels._cpu_gen(rng.clone()))
            idx, w = torch.empty(B, dtype=torch.int32), torch.empty(B)
            kernels.sumtree_sample(tree, rng, torch.tensor([size], dtype=torch.int32), torch.tensor([0.4]), idx, w)
            assert int(rng[1]) == ctr + 1
            leaf, w_ref = R.per_sample_ref(s32, m32, R.PER_SEED, ctr, size, B, P, np.float32(0.4),
                                           u01_override=uu.numpy())
            assert np.array_equal(idx.numpy(), leaf), (B, ctr)
            np.testing.assert_allclose(w.numpy(), w_ref, rtol=1e-5, atol=0)


@pytest.mark.parametrize('capacity,pattern', [c for c in R.per_cases() if R.tree_P(c[0]) <= 1024])
def test_per_replica_leaf_lies_in_its_stratum(capacity, pattern):
    """Independent float64 check of the replica: lane i's leaf l satisfies
    cum[l] - tol <= (i + u01) total / B <= cum[l + 1] + tol, cum = float64 prefix sum of the leaves,
    tol = (L + 2)^2 2^-24 total (L levels, each subtracting a stored partial sum that is itself up
    to L roundings off), and a zero-priority leaf is never returned. No case is exempt."""
    leaves, size, P, s32, m32 = _tree(capacity, pattern)
    l64 = np.zeros(P, dtype=np.float64)
    l64[:size] = leaves.astype(np.float64)
    cum = np.concatenate([[0.0], np.cumsum(l64)])
    total = cum[-1]
    L = P.bit_length() - 1
    tol = (L + 2) ** 2 * 2.0 ** -24 * total
    for B in R.PER_BATCHES:
        for ctr in _launches(B):
            leaf, _ = R.per_sample_ref(s32, m32, R.PER_SEED, ctr, size, B, P, 0.4)
            uu = R.u01(R.philox(R.PER_SEED ^ R.PER_KEY, ctr, np.arange(B), R.PER_LO1)[0]).astype(np.float64)
            u64 = (np.arange(B) + uu) * total / B
            assert (leaf >= 0).all() and (leaf < size).all()
            assert (l64[leaf] > 0).all(), (B, ctr)
            assert (cum[leaf] - tol <= u64).all() and (u64 <= cum[leaf + 1] + tol).all(), (B, ctr)


@pytest.mark.parametrize('capacity', [c for c in R.PER_CAPACITIES if c >= 2])
def test_per_edge_launch_meets_the_guard(capacity):
    """At (PER_SEED, PER_EDGE_CTR, B = 1024) the last lane's u equals the tree total; on the trees
    with zero leaves at the right edge the `right > 0` guard decides its leaf, and a walk without
    the guard ends on another one. This is the launch that makes the GPU test notice a missing guard."""
    leaves, size, P, s32, m32 = _tree(capacity, 'zeros')
    B = R.PER_EDGE_B
    uu = R.u01(R.philox(R.PER_SEED ^ R.PER_KEY, R.PER_EDGE_CTR, B - 1, R.PER_LO1)[0])
    assert (np.float32(B - 1) + uu) * (s32[1] / np.float32(B)) == s32[1]
    leaf, _, info = R.per_sample_ref(s32, m32, R.PER_SEED, R.PER_EDGE_CTR, size, B, P, 0.4, return_info=True)
    bare, _ = R.per_sample_ref(s32, m32, R.PER_SEED, R.PER_EDGE_CTR, size, B, P, 0.4, guard=False)
    assert info['guard_hits'] > 0
    assert leaves[leaf[-1]] > 0 and leaves[bare[-1]] == 0 and leaf[-1] != bare[-1]


@pytest.mark.parametrize('n,B', R.UNIFORM_CASES)
def test_uniform_replica_distinct_and_fixup_coverage(n, B):
    reached = {}
    for seed in R.UNIFORM_SEEDS:
        for ctr in range(R.UNIFORM_COUNTERS):
            v, fixup = R.draw_distinct_ref(seed, ctr, n, B)
            assert v.dtype == np.int32 and v.shape == (B,)
            assert v.min() >= 0 and v.max() < n
            if n >= B:
                assert len(set(v.tolist())) == B
            else:
                assert not fixup
            reached[seed, ctr] = fixup
    if (n, B) in [(100, 100), (64, 64)]:           # the serial fix-up runs under every seed of the GPU test
        for seed in R.UNIFORM_SEEDS:
            assert any(reached[seed, c] for c in range(R.UNIFORM_COUNTERS)), seed
    if (n, B) == (10000, 32):                      # rejection alone settles it
        assert not any(reached.values())


def test_uniform_replica_needs_the_attempt_counter():
    """A sampler whose redraws ignore the attempt counter gives other indices in the cases that redraw."""
    for n, B in [(5000, 512), (65537, 1024), (100, 100), (64, 64), (33, 32)]:
        for seed in R.UNIFORM_SEEDS:
            good, _ = R.draw_distinct_ref(seed, 0, n, B)
            bad, _ = R.draw_distinct_ref(seed, 0, n, B, redraw_attempt=0)
            assert (good != bad).any(), (n, B, seed)


def test_uniform_replica_chi_square():
    draws = [R.draw_distinct_ref(R.CHI2_SEED, c, R.CHI2_N, R.CHI2_B)[0] for c in range(R.CHI2_LAUNCHES)]
    thr = R.chi2_threshold()
    assert 131.7 < thr < 131.8                     # Wilson-Hilferty, 1 - 1e-6 quantile of chi2(63)
    chi2 = R.chi2_of(draws)
    print('replica chi2 = %.2f (threshold %.2f)' % (chi2, thr))
    assert chi2 < thr


def test_noise_replica_layout_and_moments():
    """[out0 | out1] is one stream of 2n elements; the index mapping 4q + 2h + j matters."""
    a0, a1 = R.noise_normals_ref(5, 3, 513, True)
    b0, none = R.noise_normals_ref(5, 3, 1026, False)
    assert none is None and np.array_equal(np.concatenate([a0, a1]), b0)
    c0, _ = R.noise_normals_ref(5, 3, 1026, False, swap_hj=True)
    assert np.abs(c0 - b0).max() > 1.0
    z0, z1 = R.noise_normals_ref(5, 0, 2 ** 15, True)
    z = np.concatenate([z0, z1])
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs(np.corrcoef(z0, z1)[0, 1]) < 5 / np.sqrt(n)
