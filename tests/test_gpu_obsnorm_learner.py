"""GPU tests of ``obs_norm=`` on the learners and the `Evaluator`: the default is the old path bit for bit, the learner consumes
the window normalised with the table as it stood before the update, the time-limit path classifies on the raw observations and
values the normalised ones, a rollout window with per-step `norm`, ``train()`` and the statistics' update replay from one graph,
and the `Evaluator` feeds `norm(env.z)` without touching the statistics."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import learner_ref as R
from tests import test_gpu_entropy as TE
from tests import test_gpu_learner as TG
from tests import test_gpu_timelimit as TT

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = TG.DEV


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def net_weights(torch, N, nout=16):
    gp = torch.Generator().manual_seed(0)
    rw = lambda *s: (torch.rand(*s, generator=gp) * 2 - 1) * 0.2
    return ([rw(N, 6, 48), rw(N, 48), rw(N, 48, 48), rw(N, 48), rw(N, 48, nout), rw(N, nout)],
            [rw(N, 6, 32), rw(N, 32), rw(N, 32, 32), rw(N, 32), rw(N, 32, 1), rw(N, 1)])


def networks(torch, N):
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    wa, wc = net_weights(torch, N)
    return BatchedMLP(*wa, 1, 1, device=DEV, seed=7), BatchedMLP(*wc, 0, 0, device=DEV)


def make_learner(torch, which, N, **kw):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    actor, critic = networks(torch, N)
    if which == "sa2c":
        return actor, critic, SA2CLearner(actor, critic, 0.99, **kw)
    return actor, critic, PPOLearner(actor, critic, 0.99, **{"epochs": 2, **kw})


def real_window(torch, N, G, E, T, t0):
    """A random-policy window of a batched auto_reset env into a real RolloutStorage; ``t0 [E]`` are the envs' step counters at
    its start (>= 200 - T: the time limit falls inside the window)."""
    from scalable_collision_avoidance_rl_amd import drones
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    env = drones(N, 0, [G, G], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True, device=DEV,
                 seed=11, auto_reset=True)
    env.t.copy_(torch.as_tensor(t0, dtype=env.t.dtype))
    actor, _ = networks(torch, N)
    st = RolloutStorage(env, T, actions=True)
    TG.rollout_window(env, actor, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st.z_all).all()) and bool(torch.isfinite(st.z_final).all())
    return env, st


def snapshot(actor, critic, learner, out):
    ts = [out[k] for k in sorted(out)] + [getattr(m, n) for m in (actor, critic) for n in NAMES]
    ts += [learner.actor_opt.m1, learner.actor_opt.m2, learner.critic_opt.m1, learner.critic_opt.m2, learner.G,
           learner.adv if hasattr(learner, "adv") else learner.w]
    return sorted(out), [t.clone() for t in ts]


def assert_same(torch, a, b, what):
    assert a[0] == b[0], what
    for j, (p, q) in enumerate(zip(a[1], b[1])):
        assert torch.equal(p, q), (what, j)


@pytest.fixture(scope="module")
def small_window(torch):
    """N = 5, E = 8, T = 32 at G = 5: envs 1, 2, 5 and 6 meet the time limit inside the window."""
    env, st = real_window(torch, 5, 5.0, 8, 32, [0, 180, 190, 0, 3, 175, 199, 0])
    assert int(st.done.sum()) >= 4
    return st


# 5 --------------------------------------------------------------------------------------------------------------------
CONFIGS = [("sa2c", dict()), ("sa2c", dict(lam=0.95)), ("sa2c", dict(lam=0.95, time_limit="bootstrap")),
           ("ppo", dict()), ("ppo", dict(lam=0.95)), ("ppo", dict(lam=0.95, time_limit="bootstrap")), ("ppo", dict(minibatches=4))]


@pytest.mark.parametrize("which,kw", CONFIGS, ids=[w + "-" + ("-".join(f"{k}{v}" for k, v in kw.items()) or "plain") for w, kw in CONFIGS])
def test_defaults_are_the_old_path(torch, small_window, which, kw):
    """``obs_norm=None`` against a fresh normaliser without a clamp that is never updated (the identity map returns the input's
    bits): torch.equal weights, Adam moments, G, advantages and every output after two calls; and the default path has none of
    the new buffers."""
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    st, runs = small_window, []
    for with_norm in (False, True):
        norm = ObsNormalizer(5, 6, DEV, clip=None) if with_norm else None
        actor, critic, learner = make_learner(torch, which, 5, obs_norm=norm, update_obs_norm=False, **kw)
        for _ in range(2):
            out = learner.train(st)
        torch.cuda.synchronize()
        runs.append(snapshot(actor, critic, learner, out))
        assert hasattr(learner, "_xn") == with_norm and hasattr(learner, "_xn_trunc") == (with_norm and "time_limit" in kw)
        if with_norm:
            assert float(norm.count.sum()) == 0 and learner._xn.data_ptr() != st.zbuf.data_ptr()
            assert torch.equal(learner._xn, st.z_all if "lam" in kw else st.z_pre)
    assert_same(torch, *runs, (which, kw))


# 6 --------------------------------------------------------------------------------------------------------------------
N_BIG, G_BIG, E_BIG, T_BIG = 16, 28.0, 8, 16


@pytest.fixture(scope="module")
def big_window(torch):
    """A random-policy window at G = 28: goal offsets of tens of grid units next to neighbour offsets of O(1)."""
    env, st = real_window(torch, N_BIG, G_BIG, E_BIG, T_BIG, [0] * E_BIG)
    assert float(st.z_pre.abs().max()) > 10
    return st


def fitted(torch, st, **kw):
    """A normaliser with real statistics: two `update` calls on the window's halves."""
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    norm = ObsNormalizer(st.z_pre.shape[2], st.z_pre.shape[3], DEV, **kw)
    half = st.T // 2
    norm.update(st.z_pre[:half])
    norm.update(st.z_pre[half:])
    return norm


@pytest.mark.parametrize("lam", [None, 0.95])
@pytest.mark.parametrize("which", ["sa2c", "ppo"])
def test_learner_consumes_the_window_normalised_with_the_table_before_the_update(torch, big_window, which, lam):
    """A: the learner with a fitted normaliser that it does not update.  B: a learner without one on a stand-in storage whose ring
    holds `norm(z_all)` -- the same kernel, so the same bits.  C: as A but with ``update_obs_norm=True``: the same weights and
    outputs (the update is the call's last work), and afterwards the statistics of a twin that was given `update(z_pre)`."""
    st = big_window
    T, E, N = T_BIG, E_BIG, N_BIG
    norm_a = fitted(torch, st)
    assert float(norm_a.count.min()) == T * E and float(norm_a.var.max()) > 1.0
    actor, critic, learner = make_learner(torch, which, N, lam=lam, obs_norm=norm_a, update_obs_norm=False)
    state_a = norm_a.state.clone()
    out = learner.train(st)
    torch.cuda.synchronize()
    run_a = snapshot(actor, critic, learner, out)
    assert torch.equal(norm_a.state, state_a)
    zn = fitted(torch, st).norm(st.z_all, out=torch.empty_like(st.z_all))
    assert float(zn.abs().max()) <= 10.0 and not torch.equal(zn, st.z_all)
    stand_in = SimpleNamespace(zbuf=zn, z_pre=zn[:T], z_all=zn, reward=st.reward, done=st.done, actions=st.actions, nbr_pre=st.nbr_pre)
    actor, critic, learner = make_learner(torch, which, N, lam=lam)
    out = learner.train(stand_in)
    torch.cuda.synchronize()
    assert_same(torch, run_a, snapshot(actor, critic, learner, out), "the stand-in storage")
    norm_c, twin = fitted(torch, st), fitted(torch, st)
    actor, critic, learner = make_learner(torch, which, N, lam=lam, obs_norm=norm_c)
    out = learner.train(st)
    twin.update(st.z_pre)
    torch.cuda.synchronize()
    assert_same(torch, run_a, snapshot(actor, critic, learner, out), "update_obs_norm=True")
    assert torch.equal(norm_c.state, twin.state) and torch.equal(norm_c.table, twin.table)
    assert float(norm_c.count.min()) == float(norm_c.count.max()) == 2 * T * E    # the T E pre-step rows, slot T not among them


def test_learner_refuses_a_normaliser_of_another_shape(torch):
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    for which in ("sa2c", "ppo"):
        with pytest.raises(ValueError, match="normaliser"):
            make_learner(torch, which, 5, obs_norm=ObsNormalizer(6, 6, DEV))


# 7 --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def limit_window(torch):
    """The window of tests/test_gpu_timelimit.py: arrivals at slot 0 and time-limit ends at slots 12 .. 19, N = 5, E = 64, T = 24."""
    env, st, grp, slot = TT.limit_env(torch)
    TT.zero_action_window(env, st)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st.z_all).all()) and bool(torch.isfinite(st.z_final).all())
    return st, grp


@pytest.mark.parametrize("which", ["sa2c", "ppo"])
def test_time_limit_ends_are_decided_on_the_raw_observations_and_valued_on_the_normalised(torch, limit_window, which):
    st, grp = limit_window
    T, E, N = TT.T_TL, TT.E_TL, TT.N_TL
    kw = dict(lam=0.95, time_limit="bootstrap")
    _, _, plain = make_learner(torch, which, N, **kw)
    plain.train(st)
    norm = fitted(torch, st)
    actor, critic, learner = make_learner(torch, which, N, obs_norm=norm, **kw)
    st.episode_ends()
    z_trunc = st.z_trunc.clone()
    want = critic.forward(fitted(torch, st).norm(z_trunc).view(E, N, -1)).clone()          # the PRE-update critic
    want_all = critic.forward(fitted(torch, st).norm(st.z_all).view((T + 1) * E, N, -1)).clone()
    learner.train(st)
    torch.cuda.synchronize()
    assert int((plain.ends == 1).sum()) > 0 and int((plain.ends == 2).sum()) > 0        # both kinds of end
    assert torch.equal(learner.ends, plain.ends) and torch.equal(learner.slot_t, plain.slot_t)
    assert torch.equal(learner.n_trunc, plain.n_trunc) and torch.equal(learner.n_trunc, (grp == 1).to(torch.int32))
    assert torch.equal(learner.z_trunc, z_trunc) and torch.equal(learner.z_trunc, plain.z_trunc)
    assert torch.equal(learner.V_trunc.view(E, N), want.view(E, N)) and torch.equal(learner.V_all, want_all)
    assert not torch.equal(learner.V_trunc, plain.V_trunc) and not torch.equal(learner.G, plain.G)


# 8 --------------------------------------------------------------------------------------------------------------------
def normalised_window(env, actor, st, norm):
    st.begin()
    for t in range(st.T):
        actor.sample_action(norm(env.z), env=env, act_out=st.actions[t])
        env.step(st.actions[t], into=(st, t))


def test_rollout_window_with_norm_and_train_with_update_in_one_graph(torch):
    """Per-step `norm(env.z)` -> `sample_action` -> `step(into=...)` for T steps, then `PPOLearner(obs_norm=...).train` with its
    update of the statistics, captured in ONE graph after an eager warm-up: three replays equal the eager sequence bit for bit,
    in the weights and in the normaliser's state, and every column's count grows by exactly T E per replay."""
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    N, E, T, epochs = TE.N_RS, TE.E_RS, TE.T_RS, 2

    def setup():
        norm = ObsNormalizer(N, 6, DEV)
        env, actor, critic, st, learner = TE.storage_setup(torch, epochs=epochs, obs_norm=norm)
        return env, actor, critic, st, learner, norm

    def window(env, actor, critic, st, learner, norm):
        normalised_window(env, actor, st, norm)
        return learner.train(st)

    a = setup()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = window(*a)                                   # window 1 eagerly: builds the slots and every buffer
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = window(*a)
    b = setup()
    keys = sorted(out)
    snap = lambda env, actor, critic, st, learner, norm, o: [t.clone() for t in [getattr(m, n) for m in (actor, critic) for n in NAMES] +
                                                             [learner.actor_opt.m1, learner.critic_opt.m1, st.z_pre, st.actions,
                                                              learner.logp_old, learner.adv, norm.state, norm.table] + [o[k] for k in keys]]
    ref = []
    for _ in range(4):
        o2 = window(*b)
        ref.append(snap(*b, o2))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(b[3].z_pre).all())
    for rep in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        got = snap(*a, out)
        for j, (p, q) in enumerate(zip(got, ref[rep])):
            assert torch.equal(p, q), (rep, j)
        count = a[5].count
        assert float(count.min()) == float(count.max()) == (rep + 1) * T * E
    assert float(a[5].var.max()) > 0 and all(torch.isfinite(t).all() for t in got)


# 9 --------------------------------------------------------------------------------------------------------------------
def test_evaluator_feeds_the_normalised_observation_and_never_updates(torch):
    from scalable_collision_avoidance_rl_amd import drones
    from scalable_collision_avoidance_rl_amd.evaluate import Evaluator, episode_eval
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    N, E, T = 5, 6, 200
    mk = lambda: drones(N, 0, [5, 5], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True, device=DEV,
                        seed=3, auto_reset=True)
    env, twin = mk(), mk()
    actor, critic = networks(torch, N)
    norm = ObsNormalizer(N, 6, DEV, clip=5.0)
    gen = torch.Generator().manual_seed(1)
    norm.update((torch.randn(300, N, 6, generator=gen) * 2 + 0.5).to(DEV))
    state = norm.state.clone()
    ev = Evaluator(env, actor, critic, gamma=0.99, n_bins=6, obs_norm=norm)
    tab = ev.run(1)
    torch.cuda.synchronize()
    assert torch.equal(norm.state, state)
    st = RolloutStorage(twin, T, actions=True, values=True)                   # the hand-written loop that calls norm itself
    twin.reset(renew_obstacles=False)
    st.begin()
    for t in range(T):
        z = norm(twin.z)
        critic.forward(z, out=st.values[t])
        actor.sample_action(z, env=twin, act_out=st.actions[t])
        twin.step(st.actions[t], into=(st, t))
    for name in ("reward", "true_reward", "n_coll", "done", "zbuf", "actions", "values"):
        assert torch.equal(getattr(ev.storage, name), getattr(st, name)), name
    ref = episode_eval(st.reward, st.true_reward, st.n_coll, st.done, st.values, 0.99)
    for name in ("ep_len", "ep_collisions", "ep_return", "ep_true_return", "agent_return", "agent_true_return", "mean_adv"):
        assert torch.equal(tab[name][0], ref[name]), name
    # it is not the loop on the raw observation
    plain = Evaluator(mk(), actor, critic, gamma=0.99, n_bins=6)
    plain.run(1)
    assert not torch.equal(plain.storage.actions, st.actions)
    assert torch.equal(norm.state, state)
