"""GPU tier of the composed-options tests: every row of `train_ref.ROWS` (and the two clamp rows) trains `W = 3` consecutive,
network-free windows on the device, and every window is compared with the composed float64 restatement (tests/train_ref.py)
started from the device's pre-update float32 weights of that window with the restatement's own carried float64 state -- the
convention of `test_consecutive_trains_on_a_rollout_storage_match_float64`.  The bars are the suite's own for the same quantities
(cited where they are used, not re-derived).  Then: determinism and capture of the all-on row, a change of the window's shape,
and the loop of examples/train_loop.py once on a real env.  Precision f32 only: the restatement's bars are the exact forward's."""
import numpy as np
import pytest

from tests import learner_ref as R
from tests import share_ref as S
from tests import test_gpu_ppo_guard as TGU
from tests import test_gpu_share as TSH
from tests import train_ref as TR

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = "cuda:0"
N, T, E, W, D_IN = TR.N, TR.T, TR.E, TR.W, TR.D_IN
BY_ID = {r["id"]: r for r in TR.ROWS + TR.CLAMP_ROWS}
NOT_THE_WINDOW = "the window is not the one the test is written for"


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def make_learner(torch, row, Wa, Wc, target_kl=None, **over):
    """The networks, normalisers and learner of a row on the device (``target_kl``: the constructor's value for a gated row)."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    from scalable_collision_avoidance_rl_amd.reward_norm import RewardNormalizer
    opts = TR.row_options(row)
    kind = row["kind"]
    actor, critic = BatchedMLP(*Wa, kind, kind, device=DEV), BatchedMLP(*Wc, 0, 0, device=DEV)
    obs = ObsNormalizer(N, D_IN, DEV, clip=opts["obs_clip"], eps=opts["obs_eps"]) if opts["obs_norm"] else None
    rew = (RewardNormalizer(N, opts["gamma"], DEV, scope=opts["reward_norm"], clip=opts["reward_clip"], eps=opts["reward_eps"])
           if opts["reward_norm"] is not None else None)
    kw = dict(lr_actor=opts["lr_actor"], lr_critic=opts["lr_critic"], max_norm=opts["max_norm"], rows_per_chunk=row["rows_per_chunk"],
              lam=opts["lam"], time_limit=opts["time_limit"], ent_coef=opts["ent_coef"], obs_norm=obs, share=opts["share"], reward_norm=rew)
    if row["learner"] == "ppo":
        kw.update(epochs=opts["epochs"], clip_eps=opts["clip_eps"], baseline=opts["baseline"], normalize_advantage=opts["normalize_advantage"],
                  adv_eps=opts["adv_eps"], minibatches=opts["minibatches"], shuffle_seed=opts["shuffle_seed"], target_kl=target_kl,
                  vf_clip=opts["vf_clip"])
        kw.update(over)
        return actor, critic, PPOLearner(actor, critic, opts["gamma"], **kw)
    kw.update(over)
    return actor, critic, SA2CLearner(actor, critic, opts["gamma"], **kw)


def weights_of(mlp):
    return [getattr(mlp, n).detach().cpu().clone() for n in NAMES]


def amax(t):
    return float(t.abs().max())


def close(got, ref, rtol, atol=0.0, what=""):
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), np.asarray(ref, dtype=np.float64), rtol=rtol, atol=atol, err_msg=str(what))


def compare_ppo_steps(torch, out, ref, opts, what):
    """`test_gpu_ppo_guard.compare_guarded_steps` (the per-step part of `compare_guarded_with_float64`, imported, with its bars) on
    the window's ``epochs x K`` steps, and the entropy with the bar of test_gpu_entropy.py.

    ONE kind of step is compared here instead: a whole-window (K = 1) first step with ``normalize_advantage`` and no entropy term.
    Its ratio is exactly 1, so its loss is minus the mean of the standardised advantages: exactly zero.  The restatement gives 1e-16,
    the cited atol 1e-4 max |loss| collapses to 1e-20, and no float32 sum of O(1) terms can meet it.  There, and only there, the
    bar is the sum's own rounding: the suite's plain float32 bar, 1e-5, of the mean |term| over the rows."""
    epochs, K = opts["epochs"], opts["minibatches"]
    M = T * E // K
    view = {k: v.reshape(epochs, K, N) for k, v in out.items() if v.dim() >= 2 and v.shape[0] == epochs}
    zero_loss = K == 1 and opts["normalize_advantage"] and opts["ent_coef"] == 0
    TGU.compare_guarded_steps(torch, view, ref, epochs, K, M, what, skip_actor_loss=(0,) if zero_loss else ())
    if zero_loss:
        a, (computed, _) = ref["actor"][0], ref["active"][0]
        term = a["weight"].abs().mean(0)
        assert bool(computed.all()) and torch.all(a["loss"].abs() <= 1e-12 * term), (what, "the first step's loss is not the zero sum")
        err = (view["actor_loss"][0, 0].double().cpu() - a["loss"]).abs()
        assert torch.all(err <= 1e-5 * term), (what, 0, "actor_loss", err.tolist(), term.tolist())
    if "entropy" in view:
        for j in range(epochs * K):
            on = ref["active"][j][0].nonzero().flatten()
            close(view["entropy"][j // K, j % K].cpu()[on], ref["actor"][j]["entropy"][on], 1e-5, 1e-6, what=(what, j, "entropy"))


def compare_normalisers(torch, learner, out, ref, new, win, seen, what):
    """After every window: the reward scale, moments and carry with the bars of test_gpu_rewnorm.py (count exact, mean within
    1e-10 of the largest |return| seen, m2 rtol 1e-10, scale rtol 1e-9, carry within 1e-12 of the largest |return|); the
    observation state and table with those of test_gpu_obsnorm.py (count exact, mean within 1e-10 max |x| of the column, m2 rtol
    1e-10, table rtol 1e-9)."""
    if learner.reward_norm is not None:
        seen["ret"] = max(seen.get("ret", 0.0), ref["return_maxabs"])
        state, want = learner.reward_norm.state.cpu().numpy(), new["rew"]
        assert np.array_equal(state[0], want[0]), (what, "count")
        assert np.all(np.abs(state[1] - want[1]) <= 1e-10 * seen["ret"]) and np.all(np.abs(state[2] - want[2]) <= 1e-10 * want[2]), what
        close(out["reward_scale"], ref["reward_scale"], 1e-9, what=(what, "reward_scale"))
        assert np.all(np.abs(learner.reward_norm.ret.cpu().numpy() - new["ret"]) <= 1e-12 * seen["ret"]), (what, "carry")
    if learner.obs_norm is not None:
        x = win["z_pre"].reshape(T * E, N * D_IN).double().abs().max(0).values
        seen["obs"] = x if "obs" not in seen else torch.maximum(seen["obs"], x)
        state, want = learner.obs_norm.state.cpu().view(3, -1), new["obs"]
        assert torch.equal(state[0], want[0]) and float(state[0].min()) == float(state[0].max()), (what, "count")
        assert torch.all((state[1] - want[1]).abs() <= 1e-10 * seen["obs"]) and torch.all((state[2] - want[2]).abs() <= 1e-10 * want[2].abs()), what
        from tests import obsnorm_ref as OB
        assert torch.allclose(learner.obs_norm.table.cpu().view(2, -1), OB.table(want, learner.obs_norm.eps), rtol=1e-9, atol=0), (what, "table")


def compare_ends(torch, learner, ref, what):
    for k in ("ends", "slot_t", "n_trunc", "z_trunc"):
        assert np.array_equal(getattr(learner, k).cpu().numpy(), ref[k]), (what, k)


def check_gaps(torch, ref, opts, tau, what):
    """The margin of tests/test_train_host.py on the TEACHER-FORCED table: every kl a group reaches (its crossing step included)
    at least 4 bars from the threshold."""
    _, groups = S.groups_of(opts["share"], N)
    for j, (gk, mag) in enumerate(zip(ref["group_kl"], ref["klmag"])):
        computed = ref["active"][j][0]
        for g, mem in enumerate(groups):
            if bool(computed[mem[0]]):
                gap = abs(float(gk[g]) - tau) / (1e-5 * float(mag[mem].mean()))
                assert gap >= 4.0, f"{NOT_THE_WINDOW}: {what} step {j} group {g}: kl {float(gk[g])} is {gap:.2f} bars from tau {tau}"


def compare_window(torch, row, learner, actor, critic, out, ref, new, win, opts, totals, seen, what, tau=None):
    """`_compare_window`; a bar that fails where the TEACHER-FORCED reference has a hidden pre-activation within the float32
    forward's worst-case rounding of zero (kink margin <= 1: the two forwards may have taken different relu branches) is reported
    as such.  The margin itself is a condition on the free-running chain (tests/test_train_host.py); on the device's own weights,
    and on a window whose actions come from the sampler, it is a diagnosis, not a condition: most such margins flip nothing."""
    try:
        _compare_window(torch, row, learner, actor, critic, out, ref, new, win, opts, totals, seen, what, tau)
    except AssertionError as err:
        if ref["kink"] <= 1.0:
            raise AssertionError(f"{NOT_THE_WINDOW}: {what}: the teacher-forced kink margin is {ref['kink']:.3f} of the float32 forward's "
                                 f"rounding, a relu branch may differ; the bar that failed: {err}") from err
        raise


def _compare_window(torch, row, learner, actor, critic, out, ref, new, win, opts, totals, seen, what, tau=None):
    """One window of the device against the restatement ``(ref, new)`` teacher-forced from the same pre-update weights.
    ``totals``: the running (critic steps, actor steps [N]) of the calls so far, updated in place."""
    ppo = row["learner"] == "ppo"
    share = opts["share"]
    of = torch.tensor(S.groups_of(share, N)[0])
    print(what, "teacher-forced kink margin", ref["kink"])
    # G, adv / w, logp_old: the bars of test_gpu_ppo_guard.py test 11 and of test_gpu_share.py (logp_old: test_gpu_ppo.py)
    close(learner.G, ref["G"], 1e-5, 1e-5 * amax(ref["G"]), (what, "G"))
    if opts["time_limit"] == "bootstrap":
        compare_ends(torch, learner, ref, what)
    steps_c = ref["steps"]
    if ppo:
        close(learner.adv, ref["adv"], 1e-4, 1e-4 * amax(ref["adv"]), (what, "adv"))
        close(learner.logp_old, ref["logp_old"], 1e-5, 1e-5, (what, "logp_old"))
        if opts["normalize_advantage"]:                                 # the bar of test_gpu_entropy.py
            for k in ("adv_mean", "adv_std"):
                close(out[k], ref[k], 1e-4, 1e-5 * amax(ref["adv_raw"]), (what, k))
        if tau is not None:
            check_gaps(torch, ref, opts, tau, what)
            assert out["actor_steps"].cpu().tolist() == ref["actor_steps"].tolist(), (what, "actor_steps")
        if opts["vf_clip"] is not None:
            view = out["vf_clip_fraction"].reshape(opts["epochs"] * opts["minibatches"], N)
            assert float(view[0].abs().max()) == 0.0                    # the first step sees V == v_old
        compare_ppo_steps(torch, out, ref, opts, what)
        if opts["minibatches"] > 1:
            assert np.array_equal(learner.perm.cpu().numpy(), ref["perms"][-1]), (what, "the last permutation")
        taken = ref["actor_steps"]
    else:                                                               # the bars of test_gpu_share.py's SA2C test
        close(learner.w, ref["w"], 1e-4, 1e-4 * amax(ref["w"]), (what, "w"))
        close(out["critic_loss"], ref["critic_loss"], 1e-5, what=(what, "critic_loss"))
        close(out["critic_grad_norm"], ref["critic_norm"], 1e-4, what=(what, "critic_norm"))
        close(out["actor_grad_norm"], ref["actor_norm"], 1e-4, what=(what, "actor_norm"))
        close(out["actor_loss"], ref["actor_loss"], 1e-4, 1e-4 * amax(ref["actor_loss"]), (what, "actor_loss"))
        if opts["ent_coef"] > 0:
            close(out["entropy"], ref["entropy"], 1e-5, 1e-6, (what, "entropy"))
        taken = torch.ones(N, dtype=torch.long)
    totals[0], totals[1] = totals[0] + steps_c, totals[1] + taken
    assert learner.critic_opt.steps.cpu().tolist() == [totals[0]] * N, (what, "critic steps")
    assert learner.actor_opt.steps.cpu().tolist() == totals[1].tolist(), (what, "actor steps")
    assert new["critic_steps"] == totals[0] and new["actor_steps"][of].tolist() == totals[1].tolist()
    # post-update weights: `compare_guarded_with_float64`'s sharp / loose split, times the steps of THIS window
    TGU.compare_guarded_weights(torch, critic, learner.critic_opt.lr, ref["critic_post"], ref["cm2"], torch.full((N,), steps_c), (what, "critic"))
    TGU.compare_guarded_weights(torch, actor, learner.actor_opt.lr, ref["actor_post"], ref["am2"], taken, (what, "actor"))
    compare_normalisers(torch, learner, out, ref, new, win, seen, what)
    if share is not None:
        TSH.assert_tied(torch, actor, share, (what, "actor"))
        TSH.assert_tied(torch, critic, share, (what, "critic"))
        for steps in (learner.actor_opt.steps.cpu(), learner.critic_opt.steps.cpu()):
            assert torch.equal(steps, steps[S.leaders(S.groups_of(share, N)[1])[of]]), (what, "group steps")


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r["id"] for r in TR.ROWS + TR.CLAMP_ROWS])
def test_three_windows_of_a_row_match_the_composed_float64_restatement(torch, name):
    row = BY_ID[name]
    wins, Wa, Wc = TR.row_inputs(row)
    ppo = row["learner"] == "ppo"
    gated = ppo and row["target_kl"]
    actor, critic, learner = make_learner(torch, row, Wa, Wc, target_kl=row["taus"][0] if gated else None)
    state = TR.fresh_state(Wa, Wc, TR.row_options(row))
    seen, totals = {}, [0, torch.zeros(N, dtype=torch.long)]
    for w, win in enumerate(wins):
        opts = TR.row_options(row, w)
        if gated:
            learner.target_kl = row["taus"][w]
        state = dict(state, Wa=[t.double() for t in weights_of(actor)], Wc=[t.double() for t in weights_of(critic)])
        out = learner.train(TR.storage_of(win, DEV))
        torch.cuda.synchronize()
        out = {k: v.clone() for k, v in out.items()}
        ref, new = (TR.ppo_window if ppo else TR.sa2c_window)(state, win, opts)
        compare_window(torch, row, learner, actor, critic, out, ref, new, win, opts, totals, seen, f"{name} window {w}",
                       tau=row["taus"][w] if gated else None)
        state = new


# 2 --------------------------------------------------------------------------------------------------------------------
def snapshot(torch, learner, out):
    """Everything a call leaves behind, as clones (NaN norms compare by their bits)."""
    ts = [getattr(m, n) for m in (learner.actor, learner.critic) for n in NAMES]
    ts += [learner.actor_opt.m1, learner.actor_opt.m2, learner.critic_opt.m1, learner.critic_opt.m2, learner.actor_opt.steps,
           learner.critic_opt.steps, learner.G, learner.adv, learner.logp_old, learner.perm, learner.active, learner.ends, learner.slot_t,
           learner.z_trunc, learner.obs_norm.state, learner.obs_norm.table, learner.reward_norm.state, learner.reward_norm.ret,
           learner.reward_norm.scale]
    ts += [out[k] for k in sorted(out)]
    return [t.clone() for t in ts]


def same_bits(torch, a, b):
    if a.dtype in (torch.float32, torch.float64):
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def test_the_all_on_row_is_deterministic_and_replays_from_a_captured_graph(torch):
    """The all-on PPO row with a FIXED target_kl, windows 0, 0, 1, 2: two fresh learners leave identical bits after every call; a
    third, whose last three calls are replays of ONE captured graph (after one eager call that builds the buffers; the windows are
    copied into the captured storage), equals the eager run bit for bit -- the gate's reset, the permutation counter, the reward
    carry and both normalisers' updates included.  The pattern of `test_rollout_window_and_guarded_train_in_one_graph`."""
    row = BY_ID[TR.ALL_ON["ppo"]]
    wins, Wa, Wc = TR.row_inputs(row)
    tau = row["taus"][0]
    order = [0, 0, 1, 2]
    runs = []
    for _ in range(2):
        _, _, learner = make_learner(torch, row, Wa, Wc, target_kl=tau)
        snaps = []
        for w in order:
            out = learner.train(TR.storage_of(wins[w], DEV))
            torch.cuda.synchronize()
            snaps.append(snapshot(torch, learner, out))
        runs.append(snaps)
    for call, (a, b) in enumerate(zip(*runs)):
        for j, (s, t) in enumerate(zip(a, b)):
            assert same_bits(torch, s, t), ("two fresh learners", call, j)
    assert any(bool(torch.isnan(t).any()) for snap in runs[0] for t in snap if t.is_floating_point())     # the gate did act
    _, _, learner = make_learner(torch, row, Wa, Wc, target_kl=tau)
    st = TR.storage_of({k: v.clone() for k, v in wins[0].items()}, DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = learner.train(st)                                            # call 0 eagerly: builds the learner's buffers
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(snapshot(torch, learner, out), runs[0][0])):
        assert same_bits(torch, a, b), ("the eager call", j)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = learner.train(st)
    for call, w in enumerate(order[1:], 1):
        for k, v in wins[w].items():
            getattr(st, k).copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        for j, (a, b) in enumerate(zip(snapshot(torch, learner, out), runs[0][call])):
            assert same_bits(torch, a, b), ("replay", call, j)
    assert learner.critic_opt.steps.tolist() == [4 * 8] * N


# 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,other", [("ppo", (8, 16)), ("sa2c", (8, 16)), ("ppo", (8, 12))], ids=["ppo-T", "sa2c-T", "ppo-TE"])
def test_a_change_of_the_window_shape_equals_fresh_buffers(torch, which, other):
    """One all-on learner trains on window 0, then on a window of another shape -- the first 8 steps of window 1: 128 rows, a ring
    of 144 that no longer ends on a whole chunk of 64, minibatches of 32 --, then on window 0's shape again (window 2): `_prepare`'s
    cache, its early return and every buffer it re-makes.  Reference: the same three calls, each made by a learner that has never
    seen another shape -- fresh learners fed the same sequence, the state (weights, moments, counters, both normalisers') carried
    over by hand.  A `RewardNormalizer`'s carry follows one set of envs and refuses another E by design, so the case that also changes
    E (the first 12 envs: 96 rows, minibatches of 24) runs the all-on row without ``reward_norm``."""
    T2, E2 = other
    row = BY_ID[TR.ALL_ON[which]] if E2 == E else dict(BY_ID[TR.ALL_ON[which]], reward_norm=None)
    wins, Wa, Wc = TR.row_inputs(row)
    small = {k: v[:T2 + (k == "z_all"), :E2].contiguous() for k, v in wins[1].items()}
    seq = [wins[0], small, wins[2]]
    tau = row["taus"][0] if which == "ppo" else None
    _, _, one = make_learner(torch, row, Wa, Wc, target_kl=tau)
    got = []
    for win in seq:
        out = one.train(TR.storage_of(win, DEV))
        torch.cuda.synchronize()
        got.append([t.clone() for t in [getattr(m, n) for m in (one.actor, one.critic) for n in NAMES] + [one.G] + [out[k] for k in sorted(out)]])
    prev = None
    for j, win in enumerate(seq):
        Wa_j = Wa if prev is None else weights_of(prev.actor)
        Wc_j = Wc if prev is None else weights_of(prev.critic)
        _, _, fresh = make_learner(torch, row, Wa_j, Wc_j, target_kl=tau)
        if prev is not None:
            for a, b in ((fresh.actor_opt, prev.actor_opt), (fresh.critic_opt, prev.critic_opt)):
                a.m1.copy_(b.m1), a.m2.copy_(b.m2), a.steps.copy_(b.steps)
            fresh.obs_norm.state.copy_(prev.obs_norm.state), fresh.obs_norm.table.copy_(prev.obs_norm.table)
            if fresh.reward_norm is not None:
                fresh.reward_norm.state.copy_(prev.reward_norm.state), fresh.reward_norm.scale.copy_(prev.reward_norm.scale)
                fresh.reward_norm.ret = prev.reward_norm.ret.clone()
        out = fresh.train(TR.storage_of(win, DEV))
        torch.cuda.synchronize()
        want = [getattr(m, n) for m in (fresh.actor, fresh.critic) for n in NAMES] + [fresh.G] + [out[k] for k in sorted(out)]
        for i, (a, b) in enumerate(zip(got[j], want)):
            assert same_bits(torch, a, b), (which, "call", j, i)
        prev = fresh
    assert one._shape == (T, E, N) and tuple(one.G.shape) == (T, E, N)


# 4 --------------------------------------------------------------------------------------------------------------------
def test_the_loop_of_the_training_example_once_on_a_real_env(torch):
    """The loop of examples/train_loop.py -- a real auto-reset env from `test_gpu_timelimit.limit_env`'s start, a `RolloutStorage`,
    ``sample_action(obs_norm(env.z))`` -- with the all-on PPO row minus target_kl, two windows, each compared with the restatement
    teacher-forced from the arrays the storage holds.  No `ActionShield` is in this loop.  The loop is written out here as the example
    writes it (``begin``, ``sample_action(see(env.z))``, ``env.step(into=)``, ``train``): the example script itself is still not
    executed by any test, so a change of ITS order would not be noticed here."""
    from scalable_collision_avoidance_rl_amd import drones
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    row = dict(BY_ID[TR.ALL_ON["ppo"]], target_kl=False, id="loop")
    _, Wa, Wc = TR.row_inputs(row)
    env = drones(N, 0, [TR.GRID, TR.GRID], "O", k_closest=TR.K_CLOSEST, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True,
                 device=DEV, seed=5, auto_reset=True)
    e = torch.arange(E, device=DEV)
    grp = e % 4
    pos = env.pos.clone()
    pos[grp >= 2] = env._xF + 0.01
    t0 = torch.where(grp == 1, 180 + (e // 4) % 8, torch.zeros_like(e))
    t0 = torch.where(grp == 3, torch.full_like(e, 199), t0)
    env.set_state(pos, None, t0.to(torch.int32))
    storage = RolloutStorage(env, T, actions=True)
    actor, critic, learner = make_learner(torch, row, Wa, Wc)
    actor.seed = 3
    see = learner.obs_norm
    opts = TR.row_options(row)
    state = TR.fresh_state(Wa, Wc, opts)
    seen, totals, last = {}, [0, torch.zeros(N, dtype=torch.long)], None
    for w in range(2):
        storage.begin()
        for t in range(T):
            actor.sample_action(see(env.z), env=env, act_out=storage.actions[t])
            env.step(storage.actions[t], into=(storage, t))
        torch.cuda.synchronize()
        win = {k: getattr(storage, k).detach().cpu().clone() for k in ("z_pre", "z_all", "z_final", "reward", "done", "actions", "nbr_pre")}
        for k, v in win.items():
            assert bool(torch.isfinite(v.double()).all()), (w, k)
        if last is not None:                                               # the ring runs on across the two windows
            assert torch.equal(win["z_all"][0], last), "ring slot T of window 0 is not slot 0 of window 1"
        last = win["z_all"][T].clone()
        done = win["done"].numpy() != 0
        z = win["z_final"].numpy()[done]
        dist = np.sqrt(z[..., 0].astype(np.float64) ** 2 + z[..., 1].astype(np.float64) ** 2)
        assert not dist.size or float(np.abs(dist - TR.DONE_RADIUS).min()) >= TR.END_MARGIN, f"{NOT_THE_WINDOW}: an end within 1e-4 of the radius"
        state = dict(state, Wa=[x.double() for x in weights_of(actor)], Wc=[x.double() for x in weights_of(critic)])
        out = learner.train(storage)
        torch.cuda.synchronize()
        out = {k: v.clone() for k, v in out.items()}
        ref, new = TR.ppo_window(state, win, opts)
        compare_window(torch, row, learner, actor, critic, out, ref, new, win, opts, totals, seen, f"loop window {w}")
        state = new
    assert totals[0] == 2 * opts["epochs"] * opts["minibatches"]
