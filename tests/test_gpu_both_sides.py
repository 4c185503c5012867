"""Learning from both sides of a mirrored self-play game (PPOTrainer(self_play=True, both_sides=True)): P2's
feature rows and P2's GAE, gathered by the eligible arenas (fs_ppo_features_p2 / fs_ppo_gae_p2, csrc/fs_learn.hip),
bit for bit against the torch definitions and the existing one-side calls on gathered arrays; the trainer's joint
sample table against the same table built here; which groups' P2 samples a run uses (only those that played the
learner's own weights, never a bot group); the torch learner on the same table; and two data-parallel ranks.

Bars: the kernels and the table are compared bit for bit.  fs_ppo_gae_p2 against ppo.gae uses test_gpu_learn.py's
bar for fs_ppo_gae (rtol 1e-5, atol 1e-5 x the largest advantage: one fused multiply-add against addcmul), the
bf16-actor diagnostics test_gpu_policy.py's (mean |d logp| < 0.02 and |KL| < 1e-3: P2 is the same bf16 actor on
rows of the same magnitudes; see _kl_bar for the KL estimate at this file's small sample counts), and the two
learners test_ppo_trainer_hip_step_equals_torch_step's (after Adam's first step every weight within 2 lr, at
most 1 in 1000 further apart than 1e-6)."""
import copy
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS = ("guard", "move", "move_frame", "position")


def _sim(n, seed=5, **kw):
    from footsies_gym_amd.simulator import FootsiesSim
    return FootsiesSim(n, p2_mode="external", seed=seed, **kw)


def _trainer(n, **kw):
    from footsies_gym_amd.ppo import PPOTrainer
    kw = dict(dict(horizon=8, epochs=1, minibatches=2, lr=1e-2, seed=3, self_play=True, both_sides=True), **kw)
    return PPOTrainer(_sim(n), **kw)


def _weights(tr):
    import torch
    return torch.cat([p.detach().reshape(-1) for p in list(tr.actor.parameters()) + list(tr.critic.parameters())])


def _kl_bar(n):
    """test_gpu_policy.py's |KL| < 1e-3 was set for estimates over 4 096 and more samples.  The estimate is the
    mean of n per-sample log-prob gaps; gaps of mean magnitude at most 0.02 (the other bar) have, as zero-mean
    normal values, a standard deviation of at most 0.02 sqrt(pi / 2) = 0.025, so the mean of n of them scatters
    by 0.025 / sqrt(n) around the true KL: 1.3e-3 at the 384 samples of one tick of 384 arenas, more than the bar
    itself.  The bar here is therefore 1e-3 plus four such standard errors."""
    return 1e-3 + 4 * 0.02 * (np.pi / 2) ** 0.5 / n ** 0.5


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _torch_feats(tr, first):
    """[T + 1][N][8] from the torch definitions: `first`, then obs_features of every trajectory row"""
    import torch
    from footsies_gym_amd.rollout import obs_features
    return torch.stack([first] + [obs_features({k: tr[k][t] for k in COLS}) for t in range(tr["guard"].shape[0])])


# ---------------------------------------------------------------------------------------------- features
@pytest.fixture(scope="module")
def feature_rows():
    """Six [130][2] rows of trajectory columns: a real 5-tick mirrored self-play rollout at N = 130 (one full
    group plus two arenas) and one synthetic row with positions -0.0, 0.0, +-4.6 and every guard / move byte."""
    import torch
    from footsies_gym_amd.rollout import FusedSelfPlayRollout, make_actor
    sim = _sim(130, seed=11)
    tr = sim.alloc_trajectory(5)
    FusedSelfPlayRollout(sim, make_actor(device=sim.device, seed=4), seed=2, mirror=True).rollout(5, trajectory=tr)
    dev = sim.device
    i = torch.arange(260, device=dev)
    pos = torch.tensor([-0.0, 0.0, 4.6, -4.6, 0.0, -0.0, -4.6, 4.6, 1.25, -3.5], device=dev)[i % 10]
    g = torch.Generator(device="cuda").manual_seed(7)
    extra = {"guard": (i % 256).to(torch.uint8), "move": ((i + 131) % 256).to(torch.uint8),
             "move_frame": torch.randint(0, 56, (260,), generator=g, device=dev).float(), "position": pos}
    cols = {k: torch.cat([tr[k], extra[k].view(1, 130, 2)]).contiguous() for k in COLS}
    torch.cuda.synchronize()
    for k in ("guard", "move"):
        assert set(cols[k][5].reshape(-1).tolist()) == set(range(256)), k
    return cols


def _want_features(cols):
    import torch
    from footsies_gym_amd.rollout import mirror_features, obs_features
    return mirror_features(torch.stack([obs_features({k: cols[k][r] for k in COLS}) for r in range(cols["guard"].shape[0])]))


@pytest.mark.parametrize("sel", [None, [129, 0, 5, 128, 5]])
def test_p2_features_are_the_mirrored_rows_bit_for_bit(feature_rows, sel):
    import torch
    from footsies_gym_amd.ppo import features_device
    cols = feature_rows
    dev = cols["guard"].device
    want = _want_features(cols)
    # the synthetic row holds both zeros' signs, flipped by the mirror
    signs = torch.signbit(want[5][..., 6:])[want[5][..., 6:] == 0]
    assert bool(signs.any()) and bool((~signs).any())
    st = None if sel is None else torch.tensor(sel, dtype=torch.int32, device=dev)
    n = 130 if sel is None else len(sel)
    out = torch.full((6, n, 8), 7.0, dtype=torch.float32, device=dev)
    assert features_device(cols, out, p2=True, sel=st) is out
    if sel is not None:
        want = want[:, sel]
    assert torch.equal(_bits(out), _bits(want))
    # one row at a time ([N][2] columns) is the same row
    one = torch.empty((n, 8), dtype=torch.float32, device=dev)
    features_device({k: cols[k][5] for k in COLS}, one, p2=True, sel=st)
    assert torch.equal(_bits(one), _bits(want[5]))


def test_p2_features_out_of_range_entries_are_zero_rows(feature_rows):
    import torch
    from footsies_gym_amd.ppo import features_device
    cols = feature_rows
    dev = cols["guard"].device
    sel = [129, -1, 0, 130, 5, -2**31, 2**31 - 1, 128]
    out = torch.full((6, len(sel), 8), 7.0, dtype=torch.float32, device=dev)
    features_device(cols, out, p2=True, sel=torch.tensor(sel, dtype=torch.int32, device=dev))  # (FS_OK: no raise)
    want = _want_features(cols)
    for c, a in enumerate(sel):
        if 0 <= a < 130:
            assert torch.equal(_bits(out[:, c]), _bits(want[:, a])), (c, a)
        else:
            assert torch.equal(_bits(out[:, c]), torch.zeros((6, 8), dtype=torch.int32, device=dev)), (c, a)


def test_p2_calls_refuse_bad_shapes_like_their_neighbours(feature_rows):
    import torch
    from footsies_gym_amd.ppo import features_device, gae_device
    cols = feature_rows
    dev = cols["guard"].device
    sel = torch.tensor([1, 2, 3], dtype=torch.int32, device=dev)
    out = torch.empty((6, 3, 8), dtype=torch.float32, device=dev)
    for bad in (dict(sel=sel.long()), dict(sel=sel.cpu()), dict(sel=sel.view(3, 1)), dict(sel=sel[:0]),
                dict(sel=torch.arange(6, dtype=torch.int32, device=dev)[::2])):
        with pytest.raises(ValueError, match="sel"):
            features_device(cols, out, p2=True, **bad)
    with pytest.raises(ValueError, match="sel needs p2"):
        features_device(cols, out, sel=sel)
    with pytest.raises(ValueError):
        features_device(cols, out[:, :2], p2=True, sel=sel)          # (a view, and two columns for three entries)
    with pytest.raises(ValueError):
        features_device(cols, torch.empty((6, 4, 8), device=dev), p2=True, sel=sel)
    with pytest.raises(ValueError):
        features_device(cols, out, p2=True)                           # sel=None is every arena: out [6][130][8]
    rew = torch.zeros((4, 130), dtype=torch.float64, device=dev)
    done = torch.zeros((4, 130), dtype=torch.uint8, device=dev)
    val = torch.zeros((5, 3), dtype=torch.float32, device=dev)
    gae_device(rew, done, val, 0.99, 0.95, p2=True, sel=sel)
    with pytest.raises(ValueError, match="sel needs p2"):
        gae_device(rew, done, val, 0.99, 0.95, sel=sel)
    with pytest.raises(ValueError, match="sel"):
        gae_device(rew, done, val, 0.99, 0.95, p2=True, sel=sel.long())
    with pytest.raises(ValueError):
        gae_device(rew, done, val, 0.99, 0.95, p2=True)               # sel=None: values [5][130]
    with pytest.raises(ValueError):
        gae_device(rew.float(), done, val, 0.99, 0.95, p2=True, sel=sel)


# --------------------------------------------------------------------------------------------------- GAE
GAE_N = 300


def _gae_case(T):
    """rewards f64 (mostly zero, some random, some exactly +-0.3 and +-1), dones at density ~0.1 and forced at
    t = 0, T - 1 and on both sides of every 16-tick batch seam (the batches are counted from the last tick),
    values, and a 257-entry selection with repeats that crosses a 256-thread block."""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cuda").manual_seed(9000 + T)
    N = GAE_N
    rew = torch.randn((T, N), generator=g, device=dev, dtype=torch.float64) * 0.3
    kind = torch.randint(0, 10, (T, N), generator=g, device=dev)
    rew[kind < 6] = 0.0
    for k, v in ((6, 0.3), (7, -0.3), (8, 1.0), (9, -1.0)):
        rew[kind == k] = v
    done = (torch.rand((T, N), generator=g, device=dev) < 0.1).to(torch.uint8)
    forced = {0, T - 1}
    for seam in range(T - 16, 0, -16):  # tick `seam` ends a batch, seam - 1 starts the next (or the single ticks)
        forced |= {seam, seam - 1}
    for j, t in enumerate(sorted(forced)):
        done[t, j::7] = 1
    val = torch.randn((T + 1, N), generator=g, device=dev)
    sel = (torch.arange(257, device=dev) * 7) % N
    sel[10], sel[200], sel[256] = sel[3], 299, sel[0]
    return rew, done, val, sel.to(torch.int32), sorted(forced)


@pytest.mark.parametrize("T", [1, 15, 16, 17, 33])
def test_p2_gae_is_the_one_side_launch_on_negated_gathered_arrays(T):
    import torch
    from footsies_gym_amd.ppo import gae, gae_device
    rew, done, val, sel, forced = _gae_case(T)
    assert all(bool(done[t].any()) for t in forced) and len(set(sel.tolist())) < 257 and {0, 299} <= set(sel.tolist())
    idx = sel.long()
    for s, ix in ((sel, idx), (None, torch.arange(GAE_N, device=val.device))):
        v = val[:, ix].contiguous()
        adv, ret = gae_device(rew, done, v, 0.99, 0.95, p2=True, sel=s)
        r, d = (-rew)[:, ix].contiguous(), done[:, ix].contiguous()
        one_adv, one_ret = gae_device(r, d, v, 0.99, 0.95)
        assert adv.shape == (T, ix.numel())
        assert torch.equal(_bits(adv), _bits(one_adv)) and torch.equal(_bits(ret), _bits(one_ret))
        want_adv, want_ret = gae(r.float(), v, d.float(), 0.99, 0.95)
        tol = 1e-5 * float(want_adv.abs().max())
        assert torch.allclose(adv, want_adv, rtol=1e-5, atol=tol)
        assert torch.allclose(ret, want_ret, rtol=1e-5, atol=tol)
    # the one-side launch itself is what it was: against ppo.gae on P1's own arrays, the same bar
    adv1, _ = gae_device(rew, done, val, 0.99, 0.95)
    want1, _ = gae(rew.float(), val, done.float(), 0.99, 0.95)
    assert torch.allclose(adv1, want1, rtol=1e-5, atol=1e-5 * float(want1.abs().max()))


def test_p2_gae_out_of_range_entries_are_zero_columns():
    import torch
    from footsies_gym_amd.ppo import gae_device
    T = 17
    rew, done, val, sel, _ = _gae_case(T)
    bad = {5: -1, 64: GAE_N, 255: 2**31 - 1, 256: -2**31}
    s = sel.clone()
    for c, a in bad.items():
        s[c] = a
    v = val[:, sel.long()].contiguous()
    adv, ret = gae_device(rew, done, v, 0.99, 0.95, p2=True, sel=s)
    good_adv, good_ret = gae_device(rew, done, v, 0.99, 0.95, p2=True, sel=sel)
    keep = torch.ones(257, dtype=torch.bool, device=val.device)
    keep[list(bad)] = False
    assert torch.equal(_bits(adv[:, keep]), _bits(good_adv[:, keep])) and torch.equal(_bits(ret[:, keep]), _bits(good_ret[:, keep]))
    zero = torch.zeros((T, len(bad)), dtype=torch.int32, device=val.device)
    assert torch.equal(_bits(adv[:, ~keep]), zero) and torch.equal(_bits(ret[:, ~keep]), zero)


# ------------------------------------------------------------------------------------------------- table
def _want_table(tr, feats, actions, rewards, dones, sel=None):
    """The joint table from the torch definitions and the existing one-side calls: P1's rows, then P2's of the
    arenas `sel` (a LongTensor; None: all), packed with the statistics of all the advantages."""
    import torch
    from footsies_gym_amd.ppo import gae_device, pack_rows
    from footsies_gym_amd.rollout import mirror_features
    T, N = actions.shape
    full = _torch_feats(tr.traj, feats[0])
    assert torch.equal(_bits(full), _bits(feats))
    pick = (lambda t: t) if sel is None else (lambda t: t.index_select(1, sel))
    feats2 = pick(mirror_features(full)).contiguous()
    parts = []
    for f, a, lp, r, d in ((full, actions, tr.logp, rewards, dones),
                           (feats2, pick(tr.p2_actions), pick(tr.p2_logp), pick(-rewards).contiguous(),
                            pick(dones).contiguous())):
        v, _ = tr._grad.evaluate(f.view(-1, 8))
        adv, ret = gae_device(r, d, v.view(T + 1, -1), tr.gamma, tr.lam)
        parts.append((f[:T].reshape(-1, 8), a.reshape(-1), lp.reshape(-1), adv.reshape(-1), ret.reshape(-1)))
    x, a, lp, adv, ret = (torch.cat([p[i] for p in parts]).contiguous() for i in range(5))
    return pack_rows(x, a, lp, adv, ret)


def test_the_joint_table_and_the_first_update():
    import torch
    from footsies_gym_amd.rollout import mirror_features
    T, N = 8, 384
    tr, twin = _trainer(N), _trainer(N, both_sides=False)
    old = [p.detach().clone() for p in tr.actor.parameters()]
    got, ref = tr.collect(), twin.collect()
    # storing P2's samples changes nothing of the game or of P1's samples
    assert torch.equal(tr.actions, twin.actions) and torch.equal(_bits(tr.logp), _bits(twin.logp))
    for k in tr.traj:
        assert torch.equal(tr.traj[k], twin.traj[k]), k
    assert torch.equal(_bits(got[0]), _bits(ref[0]))
    rows, gap = tr.prepare(*got)
    assert rows.shape == (2 * T * N, 12) and gap.shape == (tr.kl_ticks * N,)
    assert torch.equal(_bits(rows), _bits(_want_table(tr, *got)))
    assert bool((tr.p2_actions < 8).all())
    # P2's rows: the mirrored observation, its own sample, and the advantages centred over both sides
    assert torch.equal(_bits(rows[T * N:, :8]), _bits(mirror_features(got[0][:T]).reshape(-1, 8)))
    assert torch.equal(rows[T * N:, 8], tr.p2_actions.reshape(-1).float())
    assert abs(float(rows[:, 10].double().mean())) < 1e-5
    tr.update(*got)
    twin.update(*ref)
    assert int(tr.stats["p2_rows"]) == T * N and "p2_rows" not in twin.stats
    kl, d = float(tr.stats["p2_kl_behaviour_fp32"]), float(tr.stats["p2_logp_abs_diff"])
    print("P2 samples: KL(bf16 || fp32) %.2e, mean |d logp| %.2e (P1: %.2e, %.2e)" % (
        kl, d, float(tr.stats["kl_behaviour_fp32"]), float(tr.stats["logp_abs_diff"])))
    assert d < 0.02 and abs(kl) < _kl_bar(tr.kl_ticks * N)  # P2's behaviour log-probs are the learner's own policy's
    for v in tr.stats.values():
        assert bool(torch.isfinite(v.float()).all())
    assert torch.equal(tr.stats["mean_reward"], twin.stats["mean_reward"])  # (P1's)
    assert not torch.equal(_weights(tr), _weights(twin))  # P2's rows took part in the update
    # the opponent was refreshed, and the next rollout's P2 log-probs come from the new weights
    assert int(tr.stats["opponent_age"]) == 0
    for a, b in zip(tr.rollout.params2, tr.actor.parameters()):
        assert torch.equal(a, b.detach())
    feats = tr.collect()[0]
    x2 = mirror_features(feats[:T]).reshape(-1, 8)
    a2 = tr.p2_actions.reshape(-1).long()[:, None]
    with torch.no_grad():
        new = torch.log_softmax(tr.actor(x2), 1).gather(1, a2)[:, 0]
        before = copy.deepcopy(tr.actor)
        for p, o in zip(before.parameters(), old):
            p.copy_(o)
        stale = torch.log_softmax(before(x2), 1).gather(1, a2)[:, 0]
    behav = tr.p2_logp.reshape(-1)
    d_new, d_old = float((behav - new).abs().mean()), float((behav - stale).abs().mean())
    print("next rollout: mean |P2 logp - fp32 logp| %.2e under the new weights, %.2e under the old" % (d_new, d_old))
    assert d_new < 0.02 and d_new < d_old


# ------------------------------------------------------------------------------------- eligibility in a run
POOL = dict(opponent_pool=3, opponent_refresh=2, opponent_latest=0.5)
RUN_N, RUN_SEED = 640, 3


def _expected_groups(league):
    """Per collect of a 4-iteration run at N = 640 (5 groups), seed 3: (age, eligible groups), from the host
    functions alone -- the pool starts with one snapshot and gains one after every second update."""
    from footsies_gym_amd.rollout import bot_groups, pool_assignment
    bots = bot_groups(RUN_SEED, 0, 5, 0.4) if league else np.zeros(5, dtype=bool)
    out, pushes, taken = [], 1, 0
    for it in range(4):
        filled, newest = min(pushes, 3), (pushes - 1) % 3
        slots = pool_assignment(RUN_SEED, it, 0, 5, filled, newest, 0.5)
        age = it - taken
        out.append((age, (slots == newest) & ~bots & (age == 0)))
        if (it + 1) % 2 == 0:
            pushes, taken = pushes + 1, it + 1
    return bots, out


def _check_the_seed_gives_a_mixed_collect():
    """(host only) the run below meets what it is about: an age-0 collect with eligible and ineligible remote
    groups, with and without a league, and at least one bot group in the league"""
    for league in (False, True):
        bots, plan = _expected_groups(league)
        assert [age for age, _ in plan] == [0, 1, 0, 1]
        assert bots.any() == league
        mixed = [ok for age, ok in plan if age == 0 and ok.any() and (~ok & ~bots).any()]
        assert mixed, "no age-0 collect with eligible and ineligible remote groups"
        assert all(not (ok & bots).any() for _, ok in plan)


@pytest.mark.parametrize("league", [False, True])
def test_a_run_learns_from_exactly_the_eligible_groups(league):
    import torch
    from footsies_gym_amd.ppo import pack_rows
    from footsies_gym_amd.rollout import mirror_features
    T, N = 8, RUN_N
    _check_the_seed_gives_a_mixed_collect()
    kw = dict(POOL, opponent_bot=0.4) if league else dict(POOL)
    tr = _trainer(N, seed=RUN_SEED, **kw)
    ref = _trainer(N, seed=RUN_SEED, both_sides=False, **kw)  # (never collects: it repeats tr's P1-only updates)
    bots, plan = _expected_groups(league)
    if league:
        assert np.array_equal(tr.bots, bots)
    for it, (age, ok) in enumerate(plan):
        got = tr.collect()
        arenas = torch.from_numpy(np.flatnonzero(np.repeat(ok, 128)[:N])).to(got[0].device)
        rows, _ = tr.prepare(*got)
        assert rows.shape[0] == T * N + T * 128 * int(ok.sum()), (it, age, ok)
        if age == 0:
            assert ok.any() and tr._p2 is not None
            if tr._p2["sel"] is not None:
                assert torch.equal(tr._p2["sel"].long(), arenas)
                assert not np.repeat(bots, 128)[tr._p2["sel"].cpu().numpy()].any()
            want = mirror_features(got[0][:T]).index_select(1, arenas).reshape(-1, 8)
            assert torch.equal(_bits(rows[T * N:, :8]), _bits(want))
            assert torch.equal(_bits(rows), _bits(_want_table(tr, *got, sel=arenas)))
            tr.update(*got)
        else:  # nothing eligible: P2's samples are not stored, and the update is the P1-only trainer's
            assert tr._p2 is None and not ok.any()
            ref.actor.load_state_dict(tr.actor.state_dict())
            ref.critic.load_state_dict(tr.critic.state_dict())
            # (a copy: load_state_dict keeps tensors that already have the right dtype and device, and the two
            # optimizers would then share their moments)
            ref.opt.load_state_dict(copy.deepcopy(tr.opt.state_dict()))
            ref.gen.set_state(tr.gen.get_state())
            ref.logp.copy_(tr.logp)
            ref.traj, ref.slots = tr.traj, tr.slots
            p1_rows, _ = ref.prepare(*got)
            assert torch.equal(_bits(rows), _bits(p1_rows))
            assert torch.equal(_bits(rows), _bits(pack_rows(rows[:, :8].contiguous(), got[1].reshape(-1), tr.logp.reshape(-1),
                                                            *_p1_gae(tr, got))))
            tr.update(*got)
            ref.update(*got)
            assert torch.equal(_bits(_weights(tr)), _bits(_weights(ref)))
        assert int(tr.stats["p2_rows"]) == T * 128 * int(ok.sum())
        assert int(tr.stats["opponent_age"]) == (0 if it % 2 else 1)
        assert tr.stats["pool_episodes"].shape == (3,)
        if not ok.any():
            assert bool(torch.isnan(tr.stats["p2_logp_abs_diff"]))


def _p1_gae(tr, got):
    from footsies_gym_amd.ppo import gae_device
    feats, actions, rewards, dones = got
    T, N = actions.shape
    v, _ = tr._grad.evaluate(feats.view(-1, 8))
    adv, ret = gae_device(rewards, dones, v.view(T + 1, N), tr.gamma, tr.lam)
    return adv.reshape(-1), ret.reshape(-1)


# ----------------------------------------------------------------------------------------- the torch learner
def test_the_torch_learner_takes_the_same_table():
    import torch
    T, N, lr = 16, 1024, 1e-3
    res, tables = [], []
    for learner in ("hip", "torch"):
        tr = _trainer(N, horizon=T, minibatches=1, lr=lr, learner=learner, learner_precision="fp32")
        got = tr.collect()
        tables.append(tr.prepare(*got)[0].clone())
        tr.update(*got)
        assert int(tr.stats["p2_rows"]) == T * N
        assert float(tr.stats["p2_logp_abs_diff"]) < 0.02
        assert abs(float(tr.stats["p2_kl_behaviour_fp32"])) < _kl_bar(tr.kl_ticks * N)
        res.append([p.detach().clone() for p in list(tr.actor.parameters()) + list(tr.critic.parameters())])
    hip, tor = tables
    assert hip.shape == tor.shape == (2 * T * N, 12)
    # features, actions, behaviour log-probs: the same data (the advantages and returns rest on the two critics'
    # forward passes, which differ by fp32 rounding; the bar on them is the one on the weights below)
    assert torch.equal(_bits(hip[:, :10]), _bits(tor[:, :10]))
    print("advantage / return columns: max |hip - torch| %.2e" % float((hip[:, 10:] - tor[:, 10:]).abs().max()))
    flips = 0
    for h, t in zip(*res):
        d = (h - t).abs()
        assert float(d.max()) <= 2 * lr * 1.001
        flips += int((d > 1e-6).sum())
    total = sum(p.numel() for p in res[0])
    print("hip against torch learner on both sides' rows: %d of %d weights further apart than 1e-6" % (flips, total))
    assert flips <= total // 1000, (flips, total)


# ----------------------------------------------------------------------------------------------- two ranks
DP_N, DP_T, WORLD = 1024, 8, 2


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def worker(rank, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.simulator import FootsiesSim
    sim = FootsiesSim(DP_N, device=0, p2_mode="external", seed=0, arena_base=rank * DP_N)
    tr = PPOTrainer(sim, horizon=DP_T, epochs=1, minibatches=2, group="default", seed=rank, self_play=True,
                    both_sides=True)
    w0 = _weights(tr).cpu().numpy()
    p2_rows = []
    for _ in range(2):
        tr.iterate()
        p2_rows.append(int(tr.stats["p2_rows"]))
    q.put({"rank": rank, "w0": w0, "w2": _weights(tr).cpu().numpy(), "p2_rows": p2_rows,
           "p2_actions": tr.p2_actions.cpu().numpy()})
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_learn_from_both_sides_and_stay_identical():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in range(WORLD):
            r = q.get(timeout=240)
            got[r["rank"]] = r
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    a, b = got[0], got[1]
    assert a["w0"].tobytes() == b["w0"].tobytes() and a["w2"].tobytes() == b["w2"].tobytes()
    assert not np.array_equal(a["w0"], a["w2"])
    assert a["p2_rows"] == b["p2_rows"] == [DP_T * DP_N] * 2
    assert not np.array_equal(a["p2_actions"], b["p2_actions"])  # (different arenas on the two ranks)
