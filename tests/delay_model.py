"""FootsiesEnv's delayed-frame rule (FE:493-535) written out in numpy, and the action streams the
frame-delay tests share.

The rule, per arena (every arena is its own FootsiesEnv): reset() clears the deque and appends
frame_delay = d copies of the episode's first state, state(-1); step() appends the new state and pops
the oldest.  So the observation / info returned by the k-th step of an episode (k = 1, 2, ...) is the
undelayed one of that episode's step k - d, or the state(-1) row while k <= d; reward and
`terminated` are the new state's.  In same-step auto-reset a terminal step's final_* carry that
popped observation and the row itself is the next episode's state(-1).

`DelayRule` replays a list of calls on a frame_delay = d oracle and on a frame_delay = 0 twin and
checks the first against the rule applied to the second; it shares no code with the oracle's deque.
"""
import numpy as np

from footsies_gym_amd import _abi
from oracle.binding import hash_actions
from tests.parity_utils import assert_same

SHIFTED = ("guard", "move", "move_frame", "position", "frame", "action", "hitstun")  # observation and info
CURRENT = ("reward", "terminated", "truncated")
AR = {"same_step": _abi.FS_AUTORESET_SAME_STEP, "next_step": _abi.FS_AUTORESET_NEXT_STEP}


def hashed(seed, n_envs, steps, quiet=0):
    """([T][N], [T][N]) uint8 actions of the hashed stream; the first `quiet` steps keep only the
    direction bits (no attack, so no hit and no terminal)."""
    p1 = np.stack([hash_actions(seed, n_envs, t, 0) for t in range(steps)])
    p2 = np.stack([hash_actions(seed, n_envs, t, 1) for t in range(steps)])
    p1[:quiet] &= 3
    p2[:quiet] &= 3
    return p1, p2


class DelayRule:
    """Expected outputs of a frame_delay = d environment from its undelayed twin's.

    feed(twin_outputs, ...) after every call made on the twin; expected() then gives the delayed
    environment's outputs after the same call."""

    def __init__(self, d, same_step, created, max_calls):
        n = len(created["frame"])
        self.d, self.same, self.n = d, same_step, n
        # pool of undelayed rows: 0 = creation, 1 + e = the twin's row after call e, 1 + E + e = its final_* row
        self.E = max_calls
        self.pool = {k: np.zeros((1 + 2 * max_calls,) + np.shape(created[k]), np.asarray(created[k]).dtype)
                     for k in SHIFTED}
        for k in SHIFTED:
            self.pool[k][0] = created[k]
        self.e = 0
        self.k = np.zeros(n, np.int64)                          # steps taken in the current episode
        self.hist = np.zeros((max_calls + 1, n), np.int64)      # pool row of the episode's step k (0: state(-1))
        self.pending = np.zeros(n, bool)                        # next-step auto-reset: the next step is the reset
        self.main = np.zeros(n, np.int64)                       # pool rows of the current expected outputs
        self.final = np.zeros(n, np.int64)
        self.cur = {k: np.array(created[k], copy=True) for k in CURRENT}
        self.ar = np.arange(n)
        self.real_rows = 0          # stepped rows whose delayed frame is >= 0
        self.max_frame = -1         # the largest delayed frame
        self.first_terminal = None  # the first call with a terminal
        self.late_terminals = 0     # terminals at an arena's own step >= d
        self.real_finals = 0        # same-step terminals whose final_frame is >= 0
        self.own_steps = np.zeros(n, np.int64)

    def _store(self, tw):
        e = self.e
        for k in SHIFTED:
            self.pool[k][1 + e] = tw[k]
            self.pool[k][1 + self.E + e] = tw["final_" + k]
        self.e += 1
        return 1 + e, 1 + self.E + e

    def _start(self, who, row):
        self.k[who] = 0
        self.hist[0, who] = row
        self.pending[who] = False

    def feed_reset(self, tw, mask=None, seed_only=False):
        """The twin's outputs after reset(mask=...): the reset arenas start an episode at that row."""
        row, _ = self._store(tw)
        if seed_only:
            return
        who = np.ones(self.n, bool) if mask is None else np.asarray(mask, bool)
        self._start(who, row)
        self.main[who] = row
        self.cur["reward"][who] = 0.0
        self.cur["terminated"][who] = 0

    def feed_step(self, tw, active=None):
        """The twin's outputs after a step of the `active` arenas (all by default)."""
        row, frow = self._store(tw)
        act = np.ones(self.n, bool) if active is None else np.asarray(active, bool)
        resets = act & self.pending          # next-step auto-reset: this step is FootsiesEnv.reset
        steps = act & ~self.pending
        term = steps & (np.asarray(tw["terminated"]) != 0)
        self.k[steps] += 1
        self.own_steps[steps] += 1
        ending = term & self.same
        # the undelayed observation of this step: the final_* row when the row itself is already state(-1)
        self.hist[self.k[steps], self.ar[steps]] = np.where(ending, frow, row)[steps]
        popped = self.hist[np.maximum(self.k - self.d, 0), self.ar]
        self.main[steps & ~ending] = popped[steps & ~ending]
        self.final[ending] = popped[ending]
        self.main[ending] = row
        self.main[resets] = row
        for k in CURRENT:
            self.cur[k][act] = np.asarray(tw[k])[act]
        fr = self.pool["frame"]
        self.real_rows += int((fr[popped[steps], self.ar[steps]] >= 0).sum())
        self.max_frame = max(self.max_frame, int(fr[popped[steps], self.ar[steps]].max(initial=-1)))
        if term.any() and self.first_terminal is None:
            self.first_terminal = self.e - 1
        self.late_terminals += int((term & (self.own_steps > self.d)).sum())
        self.real_finals += int((fr[popped[ending], self.ar[ending]] >= 0).sum())
        self._start(ending | resets, row)
        self.pending[term & ~ending] = True

    def expected(self):
        out = {k: self.pool[k][self.main, self.ar] for k in SHIFTED}
        out.update({"final_" + k: self.pool[k][self.final, self.ar] for k in SHIFTED})
        out.update({k: v.copy() for k, v in self.cur.items()})
        return out


def check_rule(got, want, call, same_step):
    """`got` (a delayed environment's outputs) against DelayRule.expected(), bit for bit."""
    for k in SHIFTED + CURRENT:
        assert_same(k, want[k], got[k], call)
    if same_step:
        term = np.asarray(want["terminated"]).astype(bool)
        for k in SHIFTED:
            assert_same("final_" + k, want["final_" + k][term], np.asarray(got["final_" + k])[term], call)
