"""Test helper: NumPy replicas of the device samplers, exact where the kernels are exact.

Every stochastic decision of the HIP path comes from ``philox()`` in ``csrc/kernels/common.h``.
Philox4x32-10 is integer arithmetic, and the fp32 operations between a draw and a decision
(``(i + u01) * (total / B)``, ``u - left``, ``a + b``) hold no transcendental function and no
product-plus-sum that contraction could round differently, so these replicas must give the same
indices as the GPU bit for bit:

* ``philox`` / ``u01``: the generator and its [0, 1) mapping;
* ``draw_distinct_ref``: ``draw_distinct`` of ``sample_dev.h`` (rejection rounds, then the serial
  bitmap fix-up);
* ``per_sample_ref``: ``per_sample_lane`` of ``sumtree_dev.h``, with the descent written one level
  at a time (not the kernel's 4-levels-per-round-trip batching) and the weights in float64;
* ``noise_normals_ref``: ``noise_normals4`` of ``common.h`` as float64 Box-Muller over the same
  uniforms (the kernel's ``__logf`` / ``__sincosf`` are approximate, so this one is compared
  with a tolerance);
* ``build_tree``: consistent fp32 sum / min trees from leaf values, so a sampler test does not
  depend on the update kernels.

The case tables of the sampler tests live here too, because the CPU tests of the replicas
(``test_philox_ref.py``) run over the same cases as the GPU tests.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_S8 = np.uint64(8)

PER_KEY = 0x5bd1e995                  # per_sample_lane: key = seed ^ PER_KEY, lo1 = PER_LO1
PER_LO1 = 0x7
NOISE_KEY = 0x2545f4914f6cdd1d        # noise_normals4: key = seed ^ NOISE_KEY, lo1 = NOISE_LO1
NOISE_LO1 = 0x6e6f6973


# ------------------------------------------------------------------ generator
def philox(key64, ctr_hi, lo0, lo1):
    """Philox4x32-10 with key words (k0, k1) = (low, high) of ``key64`` and counter words
    (lo0, lo1, low of ctr_hi, high of ctr_hi). Vectorised over lo0 / lo1; returns four
    uint64 arrays holding 32-bit values."""
    key64, ctr_hi = int(key64) & (2 ** 64 - 1), int(ctr_hi) & (2 ** 64 - 1)
    lo0, lo1 = np.broadcast_arrays(np.asarray(lo0, dtype=np.uint64), np.asarray(lo1, dtype=np.uint64))
    c0, c1 = lo0 & M32, lo1 & M32
    c2 = np.full(c0.shape, ctr_hi & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(c0.shape, ctr_hi >> 32, dtype=np.uint64)
    k0, k1 = key64 & 0xFFFFFFFF, key64 >> 32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0                  # 32 x 32 -> 64 bits: no overflow
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & M32, n2, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def u01(x):
    """[0, 1) in fp32, as ``u01`` of common.h (the multiply by 2^-24 is exact)."""
    return (np.asarray(x, dtype=np.uint64) >> _S8).astype(np.float32) * np.float32(2.0 ** -24)


# ------------------------------------------------------------ uniform sampler
def _dup_of_lower(v):
    """dup[i] = some lane j < i holds v[i]."""
    dup = np.ones(v.shape, dtype=bool)
    dup[np.unique(v, return_index=True)[1]] = False
    return dup


def draw_distinct_ref(seed, ctr, n, B, redraw_attempt=None):
    """``draw_distinct(seed, ctr, n, B)``: (int32 indices [B], whether the serial fix-up ran).

    ``redraw_attempt``: None = the kernel's attempt counter; an int pins lo1 of every redraw to
    it (the defect "a sampler that ignores ctr_lo1", for checking that the cases notice it)."""
    n, B = int(n), int(B)
    lanes = np.arange(B, dtype=np.uint64)
    attempt = np.zeros(B, dtype=np.uint64)

    def draw(mask):
        lo1 = attempt[mask]
        if redraw_attempt is not None:
            lo1 = np.where(lo1 > 0, np.uint64(redraw_attempt), lo1)
        x = philox(seed, ctr, lanes[mask], lo1)[0]
        attempt[mask] += np.uint64(1)
        return ((x * np.uint64(n)) >> _S32).astype(np.int64)

    v = draw(np.ones(B, dtype=bool))
    distinct_possible = n >= B
    none = np.zeros(B, dtype=bool)
    for _ in range(64):
        dup = _dup_of_lower(v) if distinct_possible else none
        if not dup.any():
            break
        v[dup] = draw(dup)
    dup = _dup_of_lower(v) if distinct_possible else none
    fixup = bool(dup.any()) and n <= 65536
    if fixup:                                   # lane 0's serial pass over an n-bit bitmap
        used = set(v[~dup].tolist())
        for j in range(B):
            if v[j] not in v[:j]:
                continue
            c = int(v[j])
            while c in used:
                c = (c + 1) % n
            used.add(c)
            v[j] = c
    return v.astype(np.int32), fixup


# ---------------------------------------------------------------- sum trees
def tree_P(capacity):
    P = 1
    while P < capacity:
        P *= 2
    return P


def build_tree(leaves32, P):
    """fp32 (sum, min) trees [2P] over ``leaves32`` (length <= P; the leaves past it are empty:
    0 in the sum tree, +inf in the min tree). Every parent is the fp32 sum / minimum of its
    two children."""
    leaves32 = np.asarray(leaves32, dtype=np.float32)
    s = np.zeros(2 * P, dtype=np.float32)
    m = np.full(2 * P, np.inf, dtype=np.float32)
    s[P:P + leaves32.size] = leaves32
    m[P:P + leaves32.size] = leaves32
    w = P
    while w > 1:
        s[w // 2:w] = s[w:2 * w:2] + s[w + 1:2 * w:2]
        m[w // 2:w] = np.minimum(m[w:2 * w:2], m[w + 1:2 * w:2])
        w //= 2
    return s, m


def per_sample_ref(sum32, min32, seed, ctr, size, B, P, beta, u01_override=None, guard=True,
                   swap_p=False, return_info=False):
    """``per_sample_lane`` for lanes 0..B-1: (int32 leaves [B], float64 weights [B]).

    The stratified draw is fp32 in the kernel's operation order; the descent takes one level at
    a time; the weights are float64 over the fp32 tree values. ``u01_override`` replaces the
    Philox uniforms. ``guard=False`` / ``swap_p=True`` are the defects "no `right > 0` guard" and
    "p and p_min swapped", for checking that the cases notice them. ``return_info`` adds a dict
    with ``guard_hits``: how many (lane, level) decisions the guard made."""
    sum32 = np.asarray(sum32, dtype=np.float32)
    min32 = np.asarray(min32, dtype=np.float32)
    total = sum32[1]
    if u01_override is None:
        uu = u01(philox(int(seed) ^ PER_KEY, ctr, np.arange(B), PER_LO1)[0])
    else:
        uu = np.asarray(u01_override, dtype=np.float32)
    u = (np.arange(B).astype(np.float32) + uu) * (total / np.float32(B))
    assert u.dtype == np.float32
    node = np.ones(B, dtype=np.int64)
    guard_hits = 0
    L = P.bit_length() - 1
    for _ in range(L):
        left, right = sum32[2 * node], sum32[2 * node + 1]
        go = u >= left
        guard_hits += int((go & ~(right > 0)).sum())
        if guard:
            go &= right > 0
        u = np.where(go, u - left, u)
        node = 2 * node + go
    n = max(int(size), 1)
    leaf = np.minimum(node - P, n - 1)
    t64 = np.float64(total)
    p = sum32[P + leaf].astype(np.float64) / t64
    pmin = np.full(B, np.float64(min32[1]) / t64)
    if swap_p:
        p, pmin = pmin, p
    b = np.float64(beta)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = (n * p) ** -b / (n * pmin) ** -b
    if return_info:
        return leaf.astype(np.int32), w, {'guard_hits': guard_hits}
    return leaf.astype(np.int32), w


# -------------------------------------------------------------------- noise
def noise_normals_ref(seed, ctr, n, two_outputs, swap_hj=False):
    """``noise_normals4`` over q = 0 .. ceil(total / 4): (out0 [n], out1 [n] or None), float64.
    ``swap_hj`` maps the element index as 4q + 2j + h (a defect, for checking the cases)."""
    total = 2 * n if two_outputs else n
    nq = (total + 3) // 4
    r = philox(int(seed) ^ NOISE_KEY, ctr, np.arange(nq), NOISE_LO1)
    z = np.empty(4 * nq, dtype=np.float64)
    for h in range(2):
        u1 = ((r[2 * h] >> _S8).astype(np.float64) + 1.0) * 2.0 ** -24          # (0, 1]
        u2 = (r[2 * h + 1] >> _S8).astype(np.float64) * 2.0 ** -24              # [0, 1)
        rad = np.sqrt(-2.0 * np.log(u1))
        for j, zz in enumerate((rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2))):
            z[(2 * j + h if swap_hj else 2 * h + j)::4] = zz
    z = z[:total]
    return (z[:n], z[n:]) if two_outputs else (z, None)


# ------------------------------------------------------------ the case tables
PER_CAPACITIES = [1, 2, 5, 16, 32, 1000, 2 ** 11 + 3, 2 ** 20]       # L = 0, 1, 3, 4, 5, 10, 12, 20
PER_PATTERNS = ['equal', 'loguniform', 'heavy', 'zeros', 'partial']
PER_BATCHES = [1, 32, 64, 100, 1024]
PER_BETAS = [0.0, 0.4, 1.0]
PER_SEED = 7


def per_leaves(capacity, pattern):
    """(fp32 leaves [size], size) of one tree of the prioritized-sampler tests, or None where the
    pattern needs more leaves than the capacity has."""
    g = np.random.default_rng(capacity * 31 + PER_PATTERNS.index(pattern))
    C = capacity
    if pattern == 'equal':
        return np.full(C, 0.75, dtype=np.float32), C
    if pattern == 'loguniform':                          # 6 decades
        return (10.0 ** g.uniform(-3, 3, C)).astype(np.float32), C
    if C < 2:
        return None
    if pattern == 'heavy':                               # one leaf holds 99.9 % of the mass
        x = g.uniform(0.5, 1.5, C)
        k = (2 * C) // 3
        x[k] = 0.0
        x[k] = 999.0 * x.sum()
        return x.astype(np.float32), C
    if pattern == 'zeros':                               # exact zeros mid-tree and at the right edge
        x = g.uniform(0.5, 1.5, C)
        x[C // 3 + 1:C // 2 + 1] = 0.0                   # (leaf 0 stays positive at every capacity)
        x[C - max(1, C // 8):] = 0.0
        return x.astype(np.float32), C
    if pattern == 'partial':                             # size < capacity: the tail leaves are empty
        size = max(1, (2 * C) // 3)
        return g.uniform(0.5, 1.5, size).astype(np.float32), size
    raise ValueError(pattern)


def per_cases():
    return [(c, p) for c in PER_CAPACITIES for p in PER_PATTERNS if per_leaves(c, p) is not None]


# A counter at which lane 1023 draws u01 >= 1 - 2^-15 under PER_SEED: at B = 1024 its (i + u01)
# rounds to B, so u = total and the walk runs down the right edge of the tree, where only the
# `right > 0` guard keeps it out of the zero / empty leaves. An in-range draw meets the guard
# about once in 2^24 lanes, so without this launch no case would notice a missing guard (found
# by scanning counters with the replica; the CPU tests assert that the guard decides here).
PER_EDGE_CTR, PER_EDGE_B = 19273, 1024

UNIFORM_CASES = [(10000, 32), (1_000_000, 64), (5000, 512), (65537, 1024), (100, 100), (64, 64), (33, 32),
                 (40, 64), (1, 8)]
UNIFORM_SEEDS = [0, 123, 2 ** 63 - 1]
UNIFORM_COUNTERS = 3

# chi-square of the uniform sampler: n = 4096, B = 64, 400 launches, 64 bins of 64 indices.
# Threshold: the 1 - 1e-6 quantile of chi2(63) by Wilson-Hilferty,
# k (1 - 2/(9k) + z sqrt(2/(9k)))^3 with z = Phi^-1(1 - 1e-6) = 4.753424 -> 131.7
CHI2_N, CHI2_B, CHI2_LAUNCHES, CHI2_BINS, CHI2_SEED = 4096, 64, 400, 64, 2024


def chi2_threshold(k=CHI2_BINS - 1, z=4.753424):
    return k * (1.0 - 2.0 / (9.0 * k) + z * (2.0 / (9.0 * k)) ** 0.5) ** 3


def chi2_of(draws):
    """chi-square statistic of the concatenated draws over CHI2_BINS equal bins of [0, CHI2_N)."""
    counts = np.bincount(np.asarray(draws).ravel() // (CHI2_N // CHI2_BINS), minlength=CHI2_BINS)
    e = counts.sum() / CHI2_BINS
    return float(((counts - e) ** 2 / e).sum())
