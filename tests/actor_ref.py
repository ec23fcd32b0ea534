"""Test helper: an exact NumPy model of the device actor step and of the replay rings it writes.

One actor step (``actor_env_step`` + ``write_random_frame`` + ``actor_advance`` of
``csrc/kernels/actor_dev.h``; the stand-alone ``actor_step_kernel`` and the head kernels' acting
blocks all run these) is a pure function of the rng words, the Q rows, the eps words, the cursors
and the env stacks. Philox is integer arithmetic; the fp32 operations between a draw and a decision
are one subtraction per eps decrement and comparisons, so there is nothing contraction or an
approximate function could round differently (the argument of ``philox_ref.py``). ``ActorRingModel``
must therefore equal the device state bit for bit after every step: tables, stacks, cursors, eps,
rng, the env-frame counter and every byte of the frame ring.

What a step does, env e of E (all read the state as it was before the step):

* frame slots ``fslot = (f0 + 2e) % F`` (the new frame) and ``rslot = (f0 + 2e + 1) % F`` (the
  reset frame, written only when the episode ends); transition slot ``(t0 + e) % C``;
* eps decays BEFORE each roll and env e rolls the (e+1)-th time: ``eps0`` is decremented e + 1
  times by ``decay`` in fp32, each time only while ``eps > eps_min``;
* ``r = philox(seed ^ 0xA5A5A5A5, ctr, e, 1)``: ``u01(r.x) < eps`` picks the random action
  ``(r.y * A) >> 32``, else the first index of the maximum of the env's Q row; ``u01(r.z)`` below
  0.01 / 0.02 gives reward +1 / -1; ``u01(r.w) < p_done`` (both fp32) ends the episode;
* the transition's state row is the env's stack before the step and its next slot is ``fslot``;
  the stack then shifts in ``fslot``, or becomes K copies of ``rslot`` when the episode ended;
* frame bytes: call i of ``philox(seed, ctr, i, salt)`` gives bytes 16 i .. 16 i + 15 (four
  little-endian words), salt ``0x100 + 2e`` for the new frame and ``0x101 + 2e`` for the reset one;
* afterwards: eps decremented E times, ``cursor = [(t0 + E) % C, (f0 + 2E) % F, min(size + E, C)]``,
  ``size_dev`` alike, ``rng[1] = ctr + 1``, ``frames_done += E``; with a sum-tree, the E new
  transitions enter at the running max priority.

The model also keeps, for every transition, the bytes its K + 1 frames held when it was written
(the state frames as they were before the step's frame writes, the next frame after them).
``stale()`` lists the live transitions whose slots hold other bytes now: the frame ring overwrote
a frame a live transition still points at. ``frame_ring_size`` of the replay is sized so that this
never happens; the CPU tests pin that bound with this model.

The case table lives here because the CPU tests of the model (``test_actor_ref.py``) and the GPU
tests (``test_actor_ring_gpu.py``) run the same cases.
"""
import numpy as np

from philox_ref import philox, u01

ACTOR_KEY = 0xA5A5A5A5                # actor_env_step: key = seed ^ ACTOR_KEY, counter words (e, 1)
_MASK64 = 2 ** 64 - 1
F32 = np.float32


def frame_bytes(seed, ctr, salt, HW):
    """``write_random_frame``: uint8 [HW]."""
    n16 = HW // 16
    out = np.empty(HW, dtype=np.uint8)
    if n16:
        r = philox(int(seed) & _MASK64, ctr, np.arange(n16), salt)
        words = np.stack([w.astype('<u4') for w in r], axis=1)          # [n16, 4]: x, y, z, w
        out[:n16 * 16] = words.view(np.uint8).reshape(-1)
    i = np.arange(n16 * 16, HW, dtype=np.uint64)                        # (tail: HW % 16 bytes)
    out[n16 * 16:] = ((i * np.uint64(131) + np.uint64(salt)) & np.uint64(0xFF)).astype(np.uint8)
    return out


def ring_frames_old(C, K):
    """The frame ring before it was sized for its writers: right for one writer only."""
    return 2 * C + K + 8


class ActorRingModel:
    """State of E device actors and the replay they write; ``step(q)`` = one actor step."""

    def __init__(self, C, F, HW, K, E, A, seed, eps, p_done, gamma=0.99, ctr=0, frames=None, stacks=None,
                 cursor=None, per_P=0):
        assert 1 <= K <= 4 and 1 <= E <= C and 2 * E <= F
        self.C, self.F, self.HW, self.K, self.E, self.A = C, F, HW, K, E, A
        self.frames = np.zeros((F, HW), dtype=np.uint8) if frames is None else np.array(frames, dtype=np.uint8)
        assert self.frames.shape == (F, HW)
        self.state_idx = np.zeros((C, K), dtype=np.int32)
        self.next_idx = np.zeros(C, dtype=np.int32)
        self.actions = np.zeros(C, dtype=np.int32)
        self.rewards = np.zeros(C, dtype=np.float32)
        self.dones = np.zeros(C, dtype=np.float32)
        self.gammas = np.ones(C, dtype=np.float32)
        # as DeviceActor starts: env e on its own frame (slot e), duplicated K times; the cursor after them
        self.stacks = (np.repeat(np.arange(E, dtype=np.int32)[:, None], K, 1) if stacks is None
                       else np.array(stacks, dtype=np.int32))
        assert self.stacks.shape == (E, K)
        self.cursor = np.array([0, E % F, 0] if cursor is None else cursor, dtype=np.int64)
        self.size_dev = np.array([self.cursor[2]], dtype=np.int32)
        self.eps = np.array(eps, dtype=np.float32)
        self.rng = np.array([seed, ctr], dtype=np.uint64).astype(np.int64)
        self.frames_done = np.zeros(1, dtype=np.int64)
        self.p_done, self.gamma = F32(p_done), F32(gamma)
        # what each transition's K + 1 frames held when it was written
        self.rec = np.zeros((C, K + 1, HW), dtype=np.uint8)
        self.written = np.zeros(C, dtype=bool)
        self.last_slots = np.zeros(0, dtype=np.int64)       # frame slots written by the last step
        self.last_t = np.zeros(0, dtype=np.int64)           # transition slots written by the last step
        self.last_random = np.zeros(0, dtype=bool)          # which envs rolled a random action
        # prioritized replay: leaves of the sum tree (the trees follow by philox_ref.build_tree)
        self.per_P = per_P
        self.leaves = np.zeros(per_P, dtype=np.float32)
        self.leaf_set = np.zeros(per_P, dtype=bool)
        self.max_p = F32(1.0)

    # ------------------------------------------------------------------ one step
    def step(self, q=None):
        C, F, K, E, A, HW = self.C, self.F, self.K, self.E, self.A, self.HW
        t0, f0, size0 = (int(v) for v in self.cursor)
        eps0, eps_min, decay = (F32(v) for v in self.eps)
        seed, ctr = (int(v) & _MASK64 for v in self.rng.astype(np.uint64))
        r = philox(seed ^ ACTOR_KEY, ctr, np.arange(E), 1)
        ux, uz, uw = u01(r[0]), u01(r[2]), u01(r[3])
        assert ux.dtype == np.float32
        before = self.frames.copy()
        new_stacks = self.stacks.copy()
        slots, ts, rolled = [], [], []
        eps = eps0
        for e in range(E):
            fslot, rslot = (f0 + 2 * e) % F, (f0 + 2 * e + 1) % F
            if eps > eps_min:                                # decrement e + 1 of this step
                eps = F32(eps - decay)
            if ux[e] < eps:
                act = int((int(r[1][e]) * A) >> 32)
                rolled.append(True)
            else:
                row = np.asarray(q[e], dtype=np.float32)
                act, best = 0, row[0]
                for i in range(1, A):
                    if row[i] > best:
                        best, act = row[i], i
                rolled.append(False)
            reward = 1.0 if uz[e] < F32(0.01) else (-1.0 if uz[e] < F32(0.02) else 0.0)
            done = bool(uw[e] < self.p_done)
            t = (t0 + e) % C
            cur = self.stacks[e].copy()
            self.state_idx[t] = cur
            self.next_idx[t] = fslot
            self.actions[t] = act
            self.rewards[t] = reward
            self.dones[t] = 1.0 if done else 0.0
            self.gammas[t] = self.gamma
            if done:
                new_stacks[e] = rslot
            else:
                new_stacks[e, :K - 1] = cur[1:]
                new_stacks[e, K - 1] = fslot
            self.frames[fslot] = frame_bytes(seed, ctr, 0x100 + 2 * e, HW)
            slots.append(fslot)
            if done:
                self.frames[rslot] = frame_bytes(seed, ctr, 0x101 + 2 * e, HW)
                slots.append(rslot)
            ts.append(t)
        for e, t in enumerate(ts):                           # (after all of the step's frame writes)
            self.rec[t, :K] = before[self.state_idx[t]]
            self.rec[t, K] = self.frames[self.next_idx[t]]
            self.written[t] = True
        self.stacks = new_stacks
        self.eps[0] = eps                                    # E decrements in all
        ns = min(size0 + E, C)
        self.cursor[:] = [(t0 + E) % C, (f0 + 2 * E) % F, ns]
        self.size_dev[0] = ns
        self.rng[1] = np.array([(ctr + 1) & _MASK64], dtype=np.uint64).astype(np.int64)[0]
        self.frames_done[0] += E
        self.last_slots = np.array(slots, dtype=np.int64)
        self.last_t = np.array(ts, dtype=np.int64)
        self.last_random = np.array(rolled, dtype=bool)
        if self.per_P:
            self.leaves[ts] = self.max_p
            self.leaf_set[ts] = True

    # ------------------------------------------------------------------ readers
    def live(self):
        """The transition slots sampling may return: [0, size)."""
        return np.arange(int(self.cursor[2]), dtype=np.int64)

    def gather(self, idx, frames=None):
        """``replay_gather_frames``: (states, next states) uint8 [B, HW, K] of the transitions idx."""
        fr = self.frames if frames is None else frames
        idx = np.asarray(idx, dtype=np.int64)
        si = self.state_idx[idx].astype(np.int64)                                   # [B, K]
        ni = np.concatenate([si[:, 1:], self.next_idx[idx].astype(np.int64)[:, None]], 1)
        return fr[si].transpose(0, 2, 1).copy(), fr[ni].transpose(0, 2, 1).copy()

    def recorded(self, idx):
        """The same stacks from the bytes recorded when each transition was written."""
        rec = self.rec[np.asarray(idx, dtype=np.int64)]                             # [B, K + 1, HW]
        return rec[:, :self.K].transpose(0, 2, 1).copy(), rec[:, 1:].transpose(0, 2, 1).copy()

    def stack_states(self):
        """``stack_states``: uint8 [E, HW, K] of the envs' current stacks."""
        return self.frames[self.stacks.astype(np.int64)].transpose(0, 2, 1).copy()

    def stale(self, frames=None):
        """Live transitions (written by this model) whose frame slots no longer hold the bytes
        recorded when the transition was written. ``frames``: a ring to judge other than the
        model's own (the device's)."""
        fr = self.frames if frames is None else np.asarray(frames).reshape(self.F, self.HW)
        idx = self.live()
        idx = idx[self.written[idx]]
        slots = np.concatenate([self.state_idx[idx], self.next_idx[idx][:, None]], 1).astype(np.int64)
        bad = (fr[slots] != self.rec[idx]).any(axis=(1, 2))
        return idx[bad]

    def tensors(self):
        """name -> array, in the device tensors' dtypes (frames [F, HW])."""
        return dict(frames=self.frames, state_idx=self.state_idx, next_idx=self.next_idx, actions=self.actions,
                    rewards=self.rewards, dones=self.dones, gammas=self.gammas, stacks=self.stacks,
                    cursor=self.cursor, size_dev=self.size_dev, eps=self.eps, rng=self.rng,
                    frames_done=self.frames_done)


# ------------------------------------------------------------ the case tables
P_DONE = 0.3
SEED = 0x1234567
EPS_RANDOM = [1.0, 1.0, 0.0]            # every action random, no decay
EPS_GREEDY = [0.0, 0.0, 0.0]            # every action the argmax
EPS_CROSS = [0.05, 0.02, 0.004]         # E = 8: 0.05 -> ... crosses eps_min = 0.02 inside the first step
BIG_CTR = 2 ** 32 - 1                   # the high counter word changes after the first step

# (name, C, K, E, A, (H, W), eps, first counter): E = 70 is more than 64 blocks through the ticket;
# C = 23 is divided by no E > 1, so steps straddle the wrap of the transition ring
CASES = [
    ('random_e1', 24, 4, 1, 6, (4, 4), EPS_RANDOM, 0),
    ('random_e3', 23, 3, 3, 18, (4, 8), EPS_RANDOM, 0),
    ('random_e8', 24, 4, 8, 2, (4, 4), EPS_RANDOM, 0),
    ('random_e8_c23', 23, 4, 8, 6, (4, 4), EPS_RANDOM, 0),
    ('random_e70', 70 + 23, 2, 70, 6, (4, 4), EPS_RANDOM, 0),
    ('greedy_e3', 23, 2, 3, 6, (4, 4), EPS_GREEDY, 0),
    ('greedy_e8', 24, 1, 8, 18, (4, 8), EPS_GREEDY, 0),
    ('greedy_e70', 70 + 24, 4, 70, 2, (4, 4), EPS_GREEDY, 0),
    ('cross_e8', 23, 4, 8, 6, (4, 8), EPS_CROSS, 0),
    # (at eps <= 0.05 no env of 'cross_e8' happens to roll below eps; these two cross the floor at
    # eps ~ 0.5 and ~ 0.23, inside a step, with rolls on both sides of it)
    ('cross_hi_e8', 24, 2, 8, 6, (4, 4), [0.62, 0.5, 0.031], 0),
    ('cross_e3', 24, 3, 3, 2, (4, 4), [0.5, 0.23, 0.037], 0),
    ('bigctr_e8', 24, 4, 8, 18, (4, 4), [0.6, 0.1, 0.003], BIG_CTR),
    ('bigctr_e1', 23, 1, 1, 6, (4, 8), [0.5, 0.5, 0.0], BIG_CTR),
]
CASE_IDS = [c[0] for c in CASES]
BOTH_BRANCHES = ['cross_hi_e8', 'cross_e3', 'bigctr_e8', 'bigctr_e1']   # random and greedy actions in one run


def ring_frames(C, K, E):
    """The frame ring the project allocates for E device writers."""
    from dist_dqn_amd.replay.device import DeviceReplay
    return DeviceReplay.frame_ring_size(C, K, E)


def num_steps(C, F, E):
    """Enough steps to wrap the transition ring three times and the frame ring once."""
    return max(-(-3 * C // E), -(-F // (2 * E))) + 2


def case_q(name, steps, E, A):
    """Q rows [steps, E, A] of a case: exact ties, rows whose maximum is last, negative zeros,
    all-equal rows (the greedy choice must be the FIRST maximum)."""
    g = np.random.default_rng(sum(name.encode()))
    q = g.choice(np.array([-1.5, -0.0, 0.0, 0.25, 0.25, 2.0], dtype=np.float32), size=(steps, E, A))
    q[:, 0, :] = g.standard_normal((steps, A)).astype(np.float32)        # (env 0: no ties)
    if E > 1:
        q[0::3, 1, :] = 0.0
        q[0::3, 1, 0] = -0.0                                             # -0 then +0: equal, first wins
        q[1::3, 1, :] = -3.0
        q[1::3, 1, A - 1] = 7.0                                          # the maximum is last
        q[2::3, 1, :] = 1.0                                              # all equal
    if E > 2:
        q[:, 2, :] = -0.0
        q[1::2, 2, A - 1] = 0.0                                          # -0 ... +0: still the first
    return np.ascontiguousarray(q, dtype=np.float32)


def first_frames(F, HW, name):
    """The ring's bytes before the first step (random: the untouched slots are compared too)."""
    g = np.random.default_rng(sum(name.encode()) + 1)
    return g.integers(0, 256, size=(F, HW), dtype=np.uint8)


def make_model(case, F=None, per=False):
    """(model, q [steps, E, A]) of a case, on the project's ring (or a ring of F frames)."""
    from philox_ref import tree_P
    name, C, K, E, A, (H, W), eps, ctr = case
    F = ring_frames(C, K, E) if F is None else F
    m = ActorRingModel(C, F, H * W, K, E, A, SEED, eps, P_DONE, ctr=ctr, frames=first_frames(F, H * W, name),
                       per_P=tree_P(C) if per else 0)
    steps = num_steps(C, F, E)
    return m, case_q(name, steps, E, A)
