"""Every refusal a step entry point of the C ABI can return before it launches anything: the return
code, the exact fs_last_error text, and fs_steps_taken left where it was.

The texts are literals copied from csrc/fs_api.cpp, so that a change to the checks the entry points
share shows up here as a changed message, not only as a changed code.  Each refused call returns
before a kernel launch (most before the device is touched at all), so no case runs a kernel with a
bad argument.  After its refusals every handle takes one accepted call: nothing was left behind.

(The 2^40 counter refusal of the per-decision self-play calls: tests/test_gpu_wide_counters.py.)
"""
import ctypes as C

import pytest

from footsies_gym_amd import _abi

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = _abi.FS_E_INVALID, _abi.FS_E_UNSUPPORTED
DEV, MIRROR = _abi.FS_ACT_DEVICE, _abi.FS_SELFPLAY_MIRROR
MAX_TICKS = 4096  # FS_SKIP_POLICY_MAX_TICKS, as the messages print it
WEIGHTS = ("w1", "b1", "w2", "b2", "w3", "b3")

# the handles' kinds: FootsiesSim keywords
KINDS = {
    "ext": dict(p2_mode="external"),
    "bot": dict(p2_mode="bot"),
    "noop": dict(p2_mode="noop"),
    "p1bot": dict(p2_mode="bot", p1_mode="bot"),
    "p1bot_ext": dict(p2_mode="external", p1_mode="bot"),
    "delay_ext": dict(p2_mode="external", frame_delay=1),
    "delay_bot": dict(p2_mode="bot", frame_delay=1),
    "switched": dict(p2_mode="external"),  # arena 0's P2 switched to the bot (fs_set_p2_mode)
}

SKIP_REMOTE = "a remote P2 (FS_P2_EXTERNAL) must answer every frame; the fused skip runs the in-game bot or an idle P2"
SKIP_P1BOT = "P1 is the bot (FS_P1_BOT): there is no agent decision to skip to"
SKIP_DELAY = "frame_delay > 0 is not supported (the delayed queue consumes every tick's row)"
SKIP_REASONS = (("ext", SKIP_REMOTE), ("switched", SKIP_REMOTE), ("p1bot_ext", SKIP_REMOTE), ("delay_ext", SKIP_REMOTE),
                ("p1bot", SKIP_P1BOT), ("delay_bot", SKIP_DELAY))
SELF_LOCAL = ("the second actor plays a remote P2: the handle needs FS_P2_EXTERNAL (this one runs the in-game bot or an "
              "idle P2)")
SELF_REASONS = (("bot", SELF_LOCAL), ("noop", SELF_LOCAL), ("p1bot", SELF_LOCAL), ("delay_bot", SELF_LOCAL),
                ("p1bot_ext", "P1 is the bot (FS_P1_BOT), not the actor"),
                ("delay_ext", "the actors observe undelayed frames; frame_delay > 0 is not supported"),
                ("switched", "some arenas' P2 is switched to the bot (fs_set_p2_mode); switch them back first"))


class World:
    """The eight handles (2 arenas each), one zeroed device buffer the pointer arguments come from,
    a one-row trajectory and the weights of an actor."""

    def __init__(self):
        import torch
        from footsies_gym_amd._lib import lib
        from footsies_gym_amd.simulator import FootsiesSim
        self.lib = lib()
        self.sims = {k: FootsiesSim(2, seed=3, **kw) for k, kw in KINDS.items()}
        self.sims["switched"].set_p2_mode("bot", [1, 0])
        dev = self.sims["ext"].device
        self.buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
        self.D = self.buf.data_ptr()  # (256-byte aligned: the allocator's granule)
        assert self.D % 256 == 0
        self.traj = self.sims["ext"].alloc_trajectory(1)
        self.w = [torch.zeros(s, dtype=torch.float32, device=dev) for s in ((64, 8), (64,), (64, 64), (64,), (8, 64), (8,))]
        torch.cuda.synchronize()

    def handle(self, kind):
        return self.sims[kind].handle

    def pol(self, drop=None, **kw):
        return _abi.fs_policy(**{k: (None if k == drop else t.data_ptr()) for k, t in zip(WEIGHTS, self.w)}, seed=1, **kw)

    def outputs(self, drop=None):
        return _abi.fs_outputs(**{k: v.data_ptr() for k, v in self.traj.items() if k != drop})

    def refused(self, kind, fn, args, code, text):
        """One refused call: the code, the text it set (over a sentinel message) and the counter."""
        h = self.handle(kind)
        assert self.lib.fs_reset(h, None, None, 99) == INVALID and self.lib.fs_last_error(h) == b"bad flags 99"
        before = self.lib.fs_steps_taken(h)
        rc = getattr(self.lib, fn)(h, *args)
        got = self.lib.fs_last_error(h).decode()
        print("%-22s %-10s %3d %s" % (fn, kind, rc, got))
        assert (rc, got) == (code, text), (fn, kind)
        assert self.lib.fs_steps_taken(h) == before, (fn, kind)

    def close(self):
        for s in self.sims.values():
            s.close()


@pytest.fixture(scope="module")
def w():
    world = World()
    yield world
    world.close()


def ref(x):
    return None if x is None else C.byref(x)


def test_one_tick_calls(w):
    D = w.D
    for fn, kind, args, text in (
            ("fs_step", "ext", (None, D, DEV), "fs_step: p1 actions required"),
            ("fs_step", "bot", (None, None, DEV), "fs_step: p1 actions required"),
            ("fs_step", "ext", (D, None, DEV), "fs_step: p2 actions required for FS_P2_EXTERNAL"),
            ("fs_step", "p1bot_ext", (None, None, DEV), "fs_step: p2 actions required for FS_P2_EXTERNAL"),
            ("fs_step", "ext", (D, D, 2), "bad flags 2"),
            ("fs_step", "bot", (D, None, -1), "bad flags -1"),
            ("fs_step_rec", "ext", (D, D, DEV, None), "fs_step_rec: record destination required"),
            ("fs_step_rec", "delay_ext", (D, D, DEV, None), "fs_step_rec: record destination required"),
            ("fs_step_rec", "ext", (D, D, DEV, D + 516), "fs_step_rec: records must be 8-byte aligned"),
            ("fs_step_rec", "ext", (None, D, DEV, D + 512), "fs_step_rec: p1 actions required"),
            ("fs_step_rec", "ext", (D, None, DEV, D + 512), "fs_step_rec: p2 actions required for FS_P2_EXTERNAL"),
            ("fs_step_rec", "ext", (D, D, 2, D + 512), "bad flags 2"),
            # (with a delayed queue the call is fs_step + fs_pack_outputs: fs_step's texts)
            ("fs_step_rec", "delay_ext", (None, D, DEV, D + 512), "fs_step: p1 actions required"),
            ("fs_step_rec", "delay_ext", (D, None, DEV, D + 512), "fs_step: p2 actions required for FS_P2_EXTERNAL"),
            ("fs_step_rec", "delay_ext", (D, D, 2, D + 512), "bad flags 2"),
            ("fs_step_masked", "ext", (None, D, D + 64, DEV), "fs_step_masked: p1 actions and mask required"),
            ("fs_step_masked", "ext", (D, D, None, DEV), "fs_step_masked: p1 actions and mask required"),
            ("fs_step_masked", "p1bot", (None, None, None, DEV), "fs_step_masked: p1 actions and mask required"),
            ("fs_step_masked", "ext", (D, None, D + 64, DEV), "fs_step_masked: p2 actions required for FS_P2_EXTERNAL"),
            ("fs_step_masked", "ext", (D, D, D + 64, 2), "bad flags 2")):
        w.refused(kind, fn, args, INVALID, text)


def test_step_skip(w):
    D = w.D
    for kind, why in SKIP_REASONS:
        w.refused(kind, "fs_step_skip", (D, None, DEV, 8, None), UNSUPPORTED, "fs_step_skip: " + why)
    for kind in ("bot", "noop"):
        for args, text in (((D, None, 4, 8, None), "fs_step_skip: bad flags 4"),
                           ((D, None, DEV, 0, None), "fs_step_skip: max_ticks must be >= 1 (got 0)"),
                           ((None, None, DEV, 8, None), "fs_step_skip: p1 actions required to start a decision"),
                           ((None, None, 0, 8, None), "fs_step_skip: p1 actions required to start a decision")):
            w.refused(kind, "fs_step_skip", args, INVALID, text)


def test_step_n_and_packed(w):
    D = w.D
    for kind, args, text in (
            ("ext", (0, None, None, 0, None), "fs_step_n: n must be > 0"),
            ("bot", (-3, D, None, 0, None), "fs_step_n: n must be > 0"),
            ("ext", (1, D, None, 0, None), "fs_step_n: give both action arrays or neither"),
            ("ext", (1, None, D, 0, None), "fs_step_n: give both action arrays or neither"),
            ("ext", (1, None, None, 0, ref(w.outputs("reward"))), "fs_step_n: trajectory buffer missing"),
            ("bot", (1, None, None, 0, ref(w.outputs("hitstun"))), "fs_step_n: trajectory buffer missing"),
            ("ext", (1, None, None, 0, ref(w.outputs("final_move"))),
             "fs_step_n: final_* trajectory buffers required in same-step autoreset")):
        w.refused(kind, "fs_step_n", args, INVALID, text)

    def packed(lanes=D + 1024, reward=D + 2048, final_lanes=D + 3072):
        return C.byref(_abi.fs_packed_traj(lanes=lanes, reward=reward, final_lanes=final_lanes))

    unaligned = "fs_step_n_packed: lanes / final_lanes must be 16-byte, reward 8-byte aligned"
    for kind, args, text in (
            ("ext", (0, D, D, packed()), "fs_step_n_packed: n must be > 0"),
            ("ext", (1, None, D, packed()), "fs_step_n_packed: p1 action rows required"),
            ("ext", (1, D, None, packed()), "fs_step_n_packed: p2 action rows required for FS_P2_EXTERNAL"),
            ("bot", (1, D, None, None), "fs_step_n_packed: lanes and reward buffers required"),
            ("bot", (1, D, None, packed(lanes=None)), "fs_step_n_packed: lanes and reward buffers required"),
            ("bot", (1, D, None, packed(reward=None)), "fs_step_n_packed: lanes and reward buffers required"),
            ("bot", (1, D, None, packed(final_lanes=None)), "fs_step_n_packed: final_lanes required in same-step autoreset"),
            ("bot", (1, D, None, packed(lanes=D + 1032)), unaligned),
            ("bot", (1, D, None, packed(final_lanes=D + 3080)), unaligned),
            ("bot", (1, D, None, packed(reward=D + 2052)), unaligned)):
        w.refused(kind, "fs_step_n_packed", args, INVALID, text)
    for kind in ("delay_ext", "delay_bot"):
        w.refused(kind, "fs_step_n_packed", (1, D, D, packed()), UNSUPPORTED,
                  "fs_step_n_packed: frame_delay > 0 is not supported (the delayed queue reads the per-field outputs)")


def test_step_n_policy(w):
    D = w.D
    weights = "fs_step_n_policy: all six weight arrays required"
    w.refused("bot", "fs_step_n_policy", (1, None, None, None), INVALID, weights)
    for k in WEIGHTS:
        w.refused("bot", "fs_step_n_policy", (1, ref(w.pol(drop=k)), None, None), INVALID, weights)
    pol = ref(w.pol())
    w.refused("bot", "fs_step_n_policy", (0, pol, None, None), INVALID, "fs_step_n_policy: n must be > 0")
    for kind in ("p1bot", "p1bot_ext"):
        w.refused(kind, "fs_step_n_policy", (1, pol, D, None), UNSUPPORTED,
                  "fs_step_n_policy: P1 is the bot (FS_P1_BOT), not the actor")
    w.refused("ext", "fs_step_n_policy", (1, pol, None, None), INVALID,
              "fs_step_n_policy: p2 actions required for FS_P2_EXTERNAL")
    for kind in ("delay_ext", "delay_bot"):
        w.refused(kind, "fs_step_n_policy", (1, pol, D, None), UNSUPPORTED,
                  "fs_step_n_policy: the actor observes undelayed frames; frame_delay > 0 is not supported")
    # (the shared trajectory check reports under fs_step_n's name)
    w.refused("bot", "fs_step_n_policy", (1, pol, None, ref(w.outputs("reward"))), INVALID,
              "fs_step_n: trajectory buffer missing")
    w.refused("ext", "fs_step_n_policy", (1, pol, D, ref(w.outputs("final_move"))), INVALID,
              "fs_step_n: final_* trajectory buffers required in same-step autoreset")


def _trajectory_cases(call):
    """(the field a trajectory lacks, the text) under the call's own name"""
    return (("reward", call + ": trajectory buffer missing"), ("action", call + ": trajectory buffer missing"),
            ("final_move", call + ": final_* trajectory buffers required in same-step autoreset"),
            ("final_hitstun", call + ": final_* trajectory buffers required in same-step autoreset"))


def test_step_skip_policy(w):
    fn, pol = "fs_step_skip_policy", ref(w.pol())
    for kind, why in SKIP_REASONS:
        w.refused(kind, fn, (1, pol, 8, None, None), UNSUPPORTED, fn + ": " + why)
    weights = fn + ": all six weight arrays required"
    for kind in ("bot", "noop"):
        w.refused(kind, fn, (1, None, 8, None, None), INVALID, weights)
        for k in WEIGHTS:
            w.refused(kind, fn, (1, ref(w.pol(drop=k)), 8, None, None), INVALID, weights)
        w.refused(kind, fn, (0, pol, 8, None, None), INVALID, fn + ": n must be >= 1 (got 0)")
        w.refused(kind, fn, (-2, pol, 8, None, None), INVALID, fn + ": n must be >= 1 (got -2)")
        w.refused(kind, fn, (1, pol, 0, None, None), INVALID, fn + ": max_ticks must be 1 .. 4096 (got 0)")
        w.refused(kind, fn, (1, pol, MAX_TICKS + 1, None, None), INVALID, fn + ": max_ticks must be 1 .. 4096 (got 4097)")
        for drop, text in _trajectory_cases(fn):
            w.refused(kind, fn, (1, pol, 8, ref(w.outputs(drop)), None), INVALID, text)


def test_step_n_selfplay(w):
    fn, pol = "fs_step_n_selfplay", ref(w.pol())
    weights = fn + ": all six weight arrays of both actors required"
    w.refused("ext", fn, (1, None, pol, MIRROR, None), INVALID, weights)
    w.refused("ext", fn, (1, pol, None, MIRROR, None), INVALID, weights)
    for k in WEIGHTS:
        w.refused("ext", fn, (1, ref(w.pol(drop=k)), pol, MIRROR, None), INVALID, weights)
        w.refused("ext", fn, (1, pol, ref(w.pol(drop=k)), MIRROR, None), INVALID, weights)
    w.refused("bot", fn, (1, pol, None, MIRROR, None), INVALID, weights)  # (the arguments before the handle's kind)
    w.refused("ext", fn, (0, pol, pol, MIRROR, None), INVALID, fn + ": n must be > 0")
    w.refused("bot", fn, (0, pol, pol, MIRROR, None), INVALID, fn + ": n must be > 0")
    w.refused("ext", fn, (1, pol, pol, 2, None), INVALID, fn + ": bad flags 2")
    w.refused("bot", fn, (1, pol, pol, 3, None), INVALID, fn + ": bad flags 3")
    for kind, why in SELF_REASONS:
        w.refused(kind, fn, (1, pol, pol, MIRROR, None), UNSUPPORTED, fn + ": " + why)
    for drop, text in _trajectory_cases(fn):
        w.refused("ext", fn, (1, pol, pol, 0, ref(w.outputs(drop))), INVALID, text)


def test_step_skip_selfplay(w):
    fn, pol = "fs_step_skip_selfplay", ref(w.pol())
    weights = fn + ": all six weight arrays of both actors required"
    w.refused("ext", fn, (1, None, pol, MIRROR, 8, None, None), INVALID, weights)
    w.refused("ext", fn, (1, pol, None, MIRROR, 8, None, None), INVALID, weights)
    for k in WEIGHTS:
        w.refused("ext", fn, (1, ref(w.pol(drop=k)), pol, MIRROR, 8, None, None), INVALID, weights)
        w.refused("ext", fn, (1, pol, ref(w.pol(drop=k)), MIRROR, 8, None, None), INVALID, weights)
    for kind in ("ext", "bot"):  # (the arguments before the handle's kind)
        w.refused(kind, fn, (0, pol, pol, MIRROR, 8, None, None), INVALID, fn + ": n must be >= 1 (got 0)")
        w.refused(kind, fn, (1, pol, pol, MIRROR, 0, None, None), INVALID, fn + ": max_ticks must be 1 .. 4096 (got 0)")
        w.refused(kind, fn, (1, pol, pol, MIRROR, MAX_TICKS + 1, None, None), INVALID,
                  fn + ": max_ticks must be 1 .. 4096 (got 4097)")
        w.refused(kind, fn, (1, pol, pol, 2, 8, None, None), INVALID, fn + ": bad flags 2")
    for kind, why in SELF_REASONS:
        w.refused(kind, fn, (1, pol, pol, MIRROR, 8, None, None), UNSUPPORTED, fn + ": " + why)
    # P2's sample arrays are indexed with int32: 2^19 decisions x 4096 ticks x 2 arenas = 2^32 entries.
    # Refused on the count alone; the (far too small) array is never touched.
    overflow = fn + ": n * max_ticks * N = 4294967296 entries of P2's sample arrays exceed int32"
    for sample in (dict(actions_out=w.D), dict(logp_out=w.D)):
        w.refused("ext", fn, (1 << 19, pol, ref(w.pol(**sample)), MIRROR, MAX_TICKS, None, None), INVALID, overflow)
    w.refused("bot", fn, (1 << 19, pol, ref(w.pol(actions_out=w.D)), MIRROR, MAX_TICKS, None, None), UNSUPPORTED,
              fn + ": " + SELF_LOCAL)  # (the handle's kind before the count)
    for drop, text in _trajectory_cases(fn):
        w.refused("ext", fn, (1, pol, pol, 0, 8, ref(w.outputs(drop)), None), INVALID, text)


def test_every_handle_still_steps(w):
    """One accepted call per handle, after the refusals above when the file runs as a whole: a fused
    n = 1 call on the two handles that take one, a plain tick on the rest."""
    import torch
    L, D, pol = w.lib, w.D, ref(w.pol())
    for kind in KINDS:
        h = w.handle(kind)
        before = L.fs_steps_taken(h)
        if kind == "ext":
            rc = L.fs_step_n_selfplay(h, 1, pol, pol, MIRROR, ref(w.outputs()))
        elif kind == "bot":
            rc = L.fs_step_skip_policy(h, 1, pol, 1, ref(w.outputs()), None)
        else:
            rc = L.fs_step(h, D, D, DEV)
        assert rc == 0, (kind, L.fs_last_error(h))
        assert L.fs_sync(h) == 0, kind
        assert L.fs_steps_taken(h) == before + 1, kind
    torch.cuda.synchronize()
