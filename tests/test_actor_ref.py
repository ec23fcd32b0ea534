"""CPU tests of the host model of the device actor and its replay rings (tests/actor_ref.py), over
the case table the GPU tests use, and of the frame-ring bound the model pins.

The ring invariant: after every actor step, no live transition points at a frame slot that was
overwritten since the transition was written (``stale()`` is empty). It must hold on the ring
``DeviceReplay.frame_ring_size`` gives for E device writers, and it does NOT hold on the host-fed
size 2C + k + 8 once E > 1 -- which is what ``DeviceReplay.reserve_writers`` is for.
"""
import numpy as np
import pytest

import actor_ref as AR


def _run(case, F=None, per=False):
    m, q = AR.make_model(case, F, per)
    for s in range(q.shape[0]):
        yield s, m, q[s]


@pytest.mark.parametrize('case', AR.CASES, ids=AR.CASE_IDS)
def test_next_state_is_the_following_state(case):
    """s' of transition t is s of transition t + E (the same env's next step) unless t ended an
    episode; then the next state of that env is K copies of the reset slot."""
    _, C, K, E = case[:4]
    prev = None
    for s, m, q in _run(case):
        m.step(q)
        cur = (m.last_t.copy(), m.state_idx[m.last_t].copy(), m.next_idx[m.last_t].copy(), m.dones[m.last_t].copy())
        if prev is not None:
            _, si, ni, dn = prev
            for e in range(E):
                if dn[e] == 0:
                    assert np.array_equal(cur[1][e], np.concatenate([si[e, 1:], [ni[e]]]))
                else:
                    assert len(set(cur[1][e].tolist())) == 1 and cur[1][e][0] == (ni[e] + 1) % m.F
        # the envs' stacks are the next states of the transitions just written
        for e in range(E):
            want = [(cur[2][e] + 1) % m.F] * K if cur[3][e] else np.concatenate([cur[1][e, 1:], [cur[2][e]]])
            assert np.array_equal(m.stacks[e], want)
        prev = cur


@pytest.mark.parametrize('case', AR.CASES, ids=AR.CASE_IDS)
def test_slots_stay_in_range_and_size_saturates(case):
    _, C, K, E = case[:4]
    wraps_c = wraps_f = 0
    for s, m, q in _run(case):
        t0, f0 = int(m.cursor[0]), int(m.cursor[1])
        m.step(q)
        wraps_c += int(m.cursor[0]) < t0 or E == C
        wraps_f += int(m.cursor[1]) < f0
        n = int(m.cursor[2])
        assert n == min(C, (s + 1) * E) == int(m.size_dev[0])
        assert int(m.cursor[0]) == (s + 1) * E % C and int(m.cursor[1]) == (E + 2 * E * (s + 1)) % m.F
        assert int(m.frames_done[0]) == (s + 1) * E and int(m.rng[1]) == case[7] + s + 1
        for a in (m.state_idx[:n], m.next_idx[:n], m.stacks):
            assert a.min() >= 0 and a.max() < m.F
        assert m.actions[:n].min() >= 0 and m.actions[:n].max() < case[4]
        assert set(np.unique(m.rewards[:n])) <= {-1.0, 0.0, 1.0} and set(np.unique(m.dones[:n])) <= {0.0, 1.0}
    assert wraps_c >= 3 and wraps_f >= 1, (wraps_c, wraps_f)       # the table's promise


@pytest.mark.parametrize('case', AR.CASES, ids=AR.CASE_IDS)
def test_eps_schedule(case):
    """eps never drops below the floor by more than the last decrement allows, never rises, and
    stays put once it is at or below ``eps_min``; above the floor a step takes E decrements."""
    E = case[3]
    f32 = np.float32
    for s, m, q in _run(case):
        e0, emin, dec = (f32(v) for v in m.eps)
        m.step(q)
        e1 = f32(m.eps[0])
        want = e0
        for _ in range(E):
            if want > emin:
                want = f32(want - dec)
        assert e1 == want and e1 <= e0
        assert e1 > f32(emin - dec) or e1 == e0                     # at most one decrement past the floor
        if e0 <= emin:
            assert e1 == e0
        assert m.eps[1] == emin and m.eps[2] == dec


def test_eps_high_takes_E_decrements_and_orders_the_rolls():
    """With eps0 far above the floor a step leaves eps0 - E * decay (fp32, one decrement at a
    time), and env e rolls against eps0 - (e + 1) * decay: a uniform between two consecutive
    values separates them."""
    E, A, f32 = 8, 6, np.float32
    m = AR.ActorRingModel(24, AR.ring_frames(24, 4, E), 16, 4, E, A, AR.SEED, [0.5, 0.1, 0.01], AR.P_DONE)
    q = np.zeros((E, A), dtype=np.float32)
    m.step(q)
    want = f32(0.5)
    for _ in range(E):
        want = f32(want - f32(0.01))
    assert m.eps[0] == want and abs(float(want) - (0.5 - E * 0.01)) < 1e-6
    # the schedule that crosses the floor mid-step: 0.05 -> 0.046 ... 0.018 after the 8th decrement
    m = AR.ActorRingModel(24, AR.ring_frames(24, 4, E), 16, 4, E, A, AR.SEED, AR.EPS_CROSS, AR.P_DONE)
    m.step(q)
    assert f32(0.02) - f32(0.004) < m.eps[0] <= f32(0.02)
    before = m.eps[0]
    m.step(q)
    assert m.eps[0] == before
    # the rolls: env e uses the (e + 1)-th value
    r = AR.philox(AR.SEED ^ AR.ACTOR_KEY, 0, np.arange(E), 1)
    ux = AR.u01(r[0])
    m = AR.ActorRingModel(24, AR.ring_frames(24, 4, E), 16, 4, E, A, AR.SEED, [1.0, 0.0, 0.1], AR.P_DONE)
    m.step(q)
    eps_e = np.array([f32(1.0)] * E)
    for e in range(E):
        v = f32(1.0)
        for _ in range(e + 1):
            v = f32(v - f32(0.1))
        eps_e[e] = v
    assert np.array_equal(m.last_random, ux < eps_e) and m.last_random.any() and not m.last_random.all()


def test_action_mapping_and_first_maximum():
    E, A = 8, 18
    r = AR.philox(AR.SEED ^ AR.ACTOR_KEY, 5, np.arange(E), 1)
    m = AR.ActorRingModel(24, AR.ring_frames(24, 4, E), 16, 4, E, A, AR.SEED, AR.EPS_RANDOM, AR.P_DONE, ctr=5)
    m.step(None)
    want = [(int(y) * A) >> 32 for y in r[1]]
    assert m.actions[:E].tolist() == want and len(set(want)) > 2
    m = AR.ActorRingModel(24, AR.ring_frames(24, 4, E), 16, 4, E, A, AR.SEED, AR.EPS_GREEDY, AR.P_DONE)
    q = np.zeros((E, A), dtype=np.float32)
    q[0, :] = -0.0
    q[0, 7] = 0.0                       # +0 is no greater than -0
    q[1, A - 1] = 1.0                   # the maximum is last
    q[2, 3] = q[2, 9] = 2.0             # a tie
    q[3, :] = -5.0                      # all equal
    m.step(q)
    assert m.actions[:4].tolist() == [0, A - 1, 3, 0]


def test_frame_bytes_layout():
    """Call i of the generator gives bytes 16 i .. 16 i + 15 as four little-endian words."""
    b = AR.frame_bytes(AR.SEED, 3, 0x102, 32)
    r = AR.philox(AR.SEED, 3, np.arange(2), 0x102)
    for i in range(2):
        for j in range(4):
            word = int(r[j][i])
            assert b[16 * i + 4 * j:16 * i + 4 * j + 4].tolist() == [(word >> (8 * k)) & 0xFF for k in range(4)]
    assert len(set(b.tolist())) > 16
    t = AR.frame_bytes(AR.SEED, 3, 0x102, 20)
    assert np.array_equal(t[:16], b[:16]) and t[16:].tolist() == [(i * 131 + 0x102) & 0xFF for i in range(16, 20)]


def test_reset_frame_written_only_on_done():
    case = AR.CASES[AR.CASE_IDS.index('random_e8')]
    seen = set()
    for s, m, q in _run(case):
        f0 = int(m.cursor[1])
        before = m.frames.copy()
        m.step(q)
        d = m.dones[m.last_t]
        for e in range(case[3]):
            fs, rs = (f0 + 2 * e) % m.F, (f0 + 2 * e + 1) % m.F
            assert not np.array_equal(m.frames[fs], before[fs])
            assert np.array_equal(m.frames[rs], before[rs]) == (d[e] == 0)
            seen.add(float(d[e]))
        touched = np.flatnonzero((m.frames != before).any(1))
        assert set(touched.tolist()) == set(m.last_slots.tolist())
    assert seen == {0.0, 1.0}


@pytest.mark.parametrize('case', AR.CASES, ids=AR.CASE_IDS)
def test_ring_invariant_on_the_project_ring(case):
    """No live transition ever points at an overwritten frame on the ring the project allocates
    for E device writers -- after every step, and the gather of the live transitions equals the
    bytes recorded when they were written."""
    for s, m, q in _run(case):
        m.step(q)
        assert m.stale().size == 0, (s, m.stale())
    idx = m.live()
    got, want = m.gather(idx), m.recorded(idx)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize('K', [1, 2, 3, 4])
@pytest.mark.parametrize('E', [1, 2, 3, 4, 8, 23])
def test_ring_bound_is_sufficient_and_tight(K, E):
    """F = 2C + 2KE (what the bindings require) keeps the invariant with no slack at all; the
    host-fed size 2C + K + 8 loses it when it is smaller than that (episodes never end here, so
    every stack reaches K steps back)."""
    C = 23
    for F, holds in ((2 * C + 2 * K * E, True), (2 * C + 2 * K * E - 2, False)):
        m = AR.ActorRingModel(C, F, 16, K, E, 2, AR.SEED, AR.EPS_RANDOM, 0.0)
        worst = 0
        for s in range(AR.num_steps(C, F, E) + 4 * K):
            m.step(None)
            worst = max(worst, m.stale().size)
        assert (worst == 0) == holds, (F, worst)


def test_host_fed_ring_size_loses_frames_with_four_writers():
    """E = 4, K = 4, C = 64 on the old ring 2C + k + 8 = 140: after the rings wrap, live
    transitions point at frames from their future. On the ring for 4 writers: none."""
    C, K, E = 64, 4, 4
    old = AR.ring_frames_old(C, K)
    assert old == 140 and AR.ring_frames(C, K, 0) == old and old < 2 * C + 2 * K * E <= AR.ring_frames(C, K, E)
    worst = {}
    for F in (old, AR.ring_frames(C, K, E)):
        m = AR.ActorRingModel(C, F, 16, K, E, 6, AR.SEED, AR.EPS_RANDOM, AR.P_DONE)
        worst[F] = 0
        for s in range(AR.num_steps(C, F, E)):
            m.step(None)
            n = m.stale().size
            worst[F] = max(worst[F], n)
            if n:                                   # what goes wrong: the gather no longer matches
                idx = m.stale()
                assert not np.array_equal(m.gather(idx)[0], m.recorded(idx)[0])
    print('stale live transitions, worst step: old ring %d -> %d, ring for %d writers %d -> %d'
          % (old, worst[old], E, AR.ring_frames(C, K, E), worst[AR.ring_frames(C, K, E)]))
    assert worst[old] > 0 and worst[AR.ring_frames(C, K, E)] == 0, worst


def test_reserve_writers_grows_the_ring_and_keeps_its_frames():
    import torch
    from dist_dqn_amd.replay import DeviceReplay
    rep = DeviceReplay(64, (4, 4), 4, device='cpu')
    assert rep.num_frames == 140 == DeviceReplay.frame_ring_size(64, 4)       # host-fed: as before
    rep.frames.random_(0, 256)
    old = rep.frames.clone()
    rep.reserve_writers(4)
    assert rep.num_frames == rep.frames.shape[0] == 172 and rep.num_frames >= 2 * 64 + 2 * 4 * 4
    assert torch.equal(rep.frames[:140], old) and not rep.frames[140:].any()
    ptr = rep.frames.data_ptr()
    rep.reserve_writers(2)                                                    # never shrinks, never moves again
    assert rep.num_frames == 172 and rep.frames.data_ptr() == ptr


def test_table_covers_what_it_promises():
    Es = {c[3] for c in AR.CASES}
    assert Es == {1, 3, 8, 70}
    assert {c[2] for c in AR.CASES} == {1, 2, 3, 4} and {c[4] for c in AR.CASES} == {2, 6, 18}
    assert {c[5] for c in AR.CASES} == {(4, 4), (4, 8)}
    assert any(c[1] % c[3] for c in AR.CASES if c[3] > 1)          # a C that E does not divide
    assert any(c[1] == 23 for c in AR.CASES)
    # a step whose E slots straddle the wrap of C
    case = AR.CASES[AR.CASE_IDS.index('random_e8_c23')]
    assert any(m.step(q) or (np.diff(m.last_t) < 0).any() for _, m, q in _run(case))
    # the schedule case crosses eps_min inside its first step
    m, q = AR.make_model(AR.CASES[AR.CASE_IDS.index('cross_e8')])
    assert m.eps[0] > m.eps[1]
    m.step(q[0])
    assert m.eps[0] <= m.eps[1]
    for name in AR.BOTH_BRANCHES:
        rolled = np.zeros(2, dtype=np.int64)
        for _, m, q in _run(AR.CASES[AR.CASE_IDS.index(name)]):
            m.step(q)
            rolled += [m.last_random.sum(), (~m.last_random).sum()]
        assert rolled.min() > 0, (name, rolled)
    for name in ('cross_hi_e8', 'cross_e3'):                       # ... with rolls after the floor was reached
        m, q = AR.make_model(AR.CASES[AR.CASE_IDS.index(name)])
        below = [m.step(x) or (m.eps[0] <= m.eps[1] and m.last_random.any()) for x in q]
        assert any(below), name
    # the large counter crosses 2^32
    m, q = AR.make_model(AR.CASES[AR.CASE_IDS.index('bigctr_e8')])
    m.step(q[0])
    assert int(m.rng[1]) == 2 ** 32


def test_per_leaves_follow_the_new_transitions():
    case = AR.CASES[AR.CASE_IDS.index('random_e8_c23')]
    for s, m, q in _run(case, per=True):
        m.step(q)
        assert m.leaf_set.sum() == min(case[1], (s + 1) * case[3])
        assert (m.leaves[m.leaf_set] == 1.0).all() and (m.leaves[~m.leaf_set] == 0.0).all()
