"""Both `sumtree_set` kernels at the level counts where their loops change shape.

B in {32, 64} takes the one-wave climb (`sumtree_update_wave`, siblings loaded in chunks of
kSibBatch = 10 levels), B in {100, 1024} the level-synchronous kernel. Levels: 0, 1, 2 (shorter
than any chunk), 10 / 11 (one chunk exactly / one level into the second), 20 / 21 (two chunks
exactly / one level into the third; 20 is the production tree).

Instead of comparing the trees with another implementation at a tolerance, the trees are read
back and must satisfy the invariant exactly: every internal node is the fp32 sum, respectively
minimum, of its two children as read back. Written leaves are compared with (|td| + eps)^alpha
in float64 at (k + 2) 2^-24 relative: one rounding of the add, powf at k = 16 ulp (the OpenCL
full-profile bound OCML is built to meet), one for alpha and eps being fp32.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
K_ULP = 16
ALPHA, EPS = 0.6, 1e-6
CAPS = {0: 1, 1: 2, 2: 3, 10: 1000, 11: 1025, 20: 2 ** 20, 21: 2 ** 20 + 5}


def _read(tree):
    return tree.sum.cpu().numpy(), tree.min.cpu().numpy(), float(tree.max_p.cpu()[0])


def _check_ancestors(s, m, P):
    assert np.array_equal(s[1:P], s[2:2 * P:2] + s[3:2 * P:2])
    assert np.array_equal(m[1:P], np.minimum(m[2:2 * P:2], m[3:2 * P:2]))


def _batch(C, B, it, g):
    """idx with duplicates, an adjacent pair (i, i ^ 1), the first and the last slot; td with the
    batch's largest |td| on the first slot's entry (so the running max is a value that survives in
    a leaf), rising then falling over the three updates."""
    idx = g.integers(0, C, B).astype(np.int32)
    idx[1::7] = idx[0]                                   # one leaf many times
    idx[3] = min(int(idx[2]) ^ 1, C - 1)                 # siblings: their paths merge at level 1
    idx[5], idx[6] = 0, C - 1
    idx[B - 1] = idx[4]                                  # a duplicate whose winner is the last lane
    td = (g.uniform(-3, 3, B)).astype(np.float32)        # the kernel takes |td|
    if B > 64:                                           # concurrent duplicate writes: equal values
        td = (((idx.astype(np.int64) * 2654435761 + it * 40503) % 65536) / 65536.0 * 6 - 3).astype(np.float32)
    td[idx == 0] = [4.0, 5.0, 3.5][it]
    return idx, td


@pytest.mark.parametrize('B', [32, 64, 100, 1024])
@pytest.mark.parametrize('levels', sorted(CAPS))
def test_sumtree_set_levels(levels, B):
    from dist_dqn_amd.replay.sumtree import DeviceSumTree
    C = CAPS[levels]
    tree = DeviceSumTree(C, DEV)
    P = tree.P
    assert P == 1 << levels
    tree.set_max_priority(torch.arange(C, dtype=torch.int32, device=DEV))
    s, m, mp = _read(tree)
    assert mp == 1.0 and (s[P:P + C] == 1.0).all() and (m[P:P + C] == 1.0).all()
    assert (s[P + C:] == 0).all() and np.isinf(m[P + C:]).all()
    _check_ancestors(s, m, P)
    g = np.random.default_rng(levels * 10 + B)
    bound = (K_ULP + 2) * 2.0 ** -24
    peaks = []
    for it in range(3):
        idx, td = _batch(C, B, it, g)
        tree.update(torch.from_numpy(idx).to(DEV), torch.from_numpy(td).to(DEV), ALPHA, EPS)
        s2, m2, mp2 = _read(tree)
        # leaves: the last batch position wins a duplicated leaf (B > 64: duplicates are equal)
        want = {}
        for j in range(B):
            want[int(idx[j])] = (abs(np.float64(td[j])) + np.float64(np.float32(EPS))) ** np.float64(np.float32(ALPHA))
        leaf = np.fromiter(want.keys(), dtype=np.int64)
        ref = np.fromiter(want.values(), dtype=np.float64)
        got = s2[P + leaf].astype(np.float64)
        assert (np.abs(got - ref) <= bound * ref).all(), (it, float((np.abs(got - ref) / ref).max() / bound))
        assert np.array_equal(m2[P + leaf], s2[P + leaf])
        untouched = np.ones(P, dtype=bool)
        untouched[leaf] = False
        assert np.array_equal(s2[P:][untouched], s[P:][untouched])
        assert np.array_equal(m2[P:][untouched], m[P:][untouched])
        _check_ancestors(s2, m2, P)
        assert mp2 == max(mp, float(s2[P + leaf].max()))
        s, m, mp = s2, m2, mp2
        peaks.append(mp)
    # a running max: the second update's 5^alpha outlives the third, which rewrites that leaf lower
    assert peaks[0] < peaks[1] == peaks[2] and float(s[P]) < peaks[2]
