"""GPU tests of ``reward_norm=`` on the learners: a learner with a `RewardNormalizer` equals, bit for bit, a learner without one
that is trained on a copy of the storage whose rewards were normalised by the same kernels beforehand; ``storage.reward`` is
never written; the default is the old path; and a rollout window with ``train()``, both normalisers and their updates replays
from one captured graph."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_gpu_learner as TG
from tests import test_gpu_obsnorm_learner as OL

pytestmark = pytest.mark.gpu
DEV = TG.DEV
N, E, T = 5, 8, 32


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def window(torch):
    """N = 5, E = 8, T = 32 at G = 5: envs 1, 2, 5 and 6 meet the time limit inside the window."""
    env, st = OL.real_window(torch, N, 5.0, E, T, [0, 180, 190, 0, 3, 175, 199, 0])
    assert int(st.done.sum()) >= 4
    return st


def rnorm(**kw):
    from scalable_collision_avoidance_rl_amd.reward_norm import RewardNormalizer
    return RewardNormalizer(N, 0.99, DEV, **kw)


def snapshot(actor, critic, learner, out):
    out = {k: v for k, v in out.items() if k != "reward_scale"}
    return OL.snapshot(actor, critic, learner, out)


VARIANTS = [dict(), dict(lam=0.95), dict(lam=0.95, time_limit="bootstrap")]
IDS = ["plain", "lam", "lam-bootstrap"]


@pytest.mark.parametrize("kw", VARIANTS, ids=IDS)
@pytest.mark.parametrize("which", ["sa2c", "ppo"])
def test_learner_equals_a_learner_on_host_normalised_rewards(torch, window, which, kw):
    """A: ``reward_norm=`` (team scope), two calls on the window.  B: no normaliser; before each call a twin normaliser is given
    the window and its `norm(reward)` stands in for the storage's reward.  Same kernels in the same order: the same bits in every
    output, weight, Adam moment, G and advantage.  The storage's own reward is untouched."""
    st = window
    raw = st.reward.clone()
    norm = rnorm()
    actor, critic, learner = OL.make_learner(torch, which, N, reward_norm=norm, **kw)
    for _ in range(2):
        out = learner.train(st)
    torch.cuda.synchronize()
    assert torch.equal(st.reward, raw)
    assert out["reward_scale"].data_ptr() == norm.scale.data_ptr() and tuple(out["reward_scale"].shape) == (N,)
    assert float(norm.count.sum()) == 2 * T * E * N and float((norm.scale - 1).abs().min()) > 0
    if "time_limit" in kw:
        assert int(learner.n_trunc.sum()) > 0                             # the window has time-limit ends
    run_a = snapshot(actor, critic, learner, out)

    twin = rnorm()
    rn = torch.empty_like(st.reward)
    stand_in = SimpleNamespace(zbuf=st.zbuf, z_pre=st.z_pre, z_all=st.z_all, z_final=st.z_final, reward=rn, done=st.done,
                               actions=st.actions, nbr_pre=st.nbr_pre)
    actor, critic, plain = OL.make_learner(torch, which, N, **kw)
    for _ in range(2):
        twin.update(st.reward, st.done)
        twin.norm(st.reward, out=rn)
        out = plain.train(stand_in)
    torch.cuda.synchronize()
    assert "reward_scale" not in out and not torch.equal(rn, raw)
    assert torch.equal(learner._rn, rn) and learner._rn.data_ptr() != st.reward.data_ptr()
    OL.assert_same(torch, run_a, snapshot(actor, critic, plain, out), (which, kw))
    assert torch.equal(norm.state, twin.state) and torch.equal(norm.scale, twin.scale) and torch.equal(norm.ret, twin.ret)
    # normalised units: the critic's target is O(1) where the raw returns are not
    raw_learner = OL.make_learner(torch, which, N, **kw)[2]
    raw_learner.train(st)
    assert float(raw_learner.G.abs().max()) > 3 * float(learner.G.abs().max())


@pytest.mark.parametrize("which", ["sa2c", "ppo"])
def test_update_reward_norm_false_leaves_the_statistics_alone(torch, window, which):
    st = window
    norm = rnorm().update(st.reward, st.done)
    state, scale, ret = norm.state.clone(), norm.scale.clone(), norm.ret.clone()
    actor, critic, learner = OL.make_learner(torch, which, N, reward_norm=norm, update_reward_norm=False)
    out = learner.train(st)
    torch.cuda.synchronize()
    assert torch.equal(norm.state, state) and torch.equal(norm.scale, scale) and torch.equal(norm.ret, ret)
    assert torch.equal(out["reward_scale"], scale) and torch.equal(learner._rn, rnorm().update(st.reward, st.done).norm(st.reward))


@pytest.mark.parametrize("kw", VARIANTS, ids=IDS)
@pytest.mark.parametrize("which", ["sa2c", "ppo"])
def test_default_is_the_path_without_the_argument(torch, window, which, kw):
    st, runs = window, []
    for extra in (dict(), dict(reward_norm=None)):
        actor, critic, learner = OL.make_learner(torch, which, N, **kw, **extra)
        for _ in range(2):
            out = learner.train(st)
        torch.cuda.synchronize()
        assert "reward_scale" not in out and not hasattr(learner, "_rn") and learner.reward_norm is None
        runs.append(OL.snapshot(actor, critic, learner, out))
    OL.assert_same(torch, *runs, (which, kw))


def test_learner_refuses_a_normaliser_that_does_not_fit(torch):
    from scalable_collision_avoidance_rl_amd.reward_norm import RewardNormalizer
    for which in ("sa2c", "ppo"):
        with pytest.raises(ValueError, match="reward normaliser"):
            OL.make_learner(torch, which, N, reward_norm=RewardNormalizer(N + 1, 0.99, DEV))


def test_rollout_window_and_train_with_both_normalisers_in_one_graph(torch):
    """Per-step `obs_norm(env.z)` -> `sample_action` -> `step(into=...)` for T steps, then `PPOLearner(obs_norm=, reward_norm=)
    .train`, captured in ONE graph after an eager warm-up: two replays equal the eager sequence of three windows bit for bit, in
    the weights, both normalisers' statistics and the return carry."""
    from scalable_collision_avoidance_rl_amd import drones
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    Tc, Ec = 12, 16

    def setup():
        env = drones(N, 0, [5, 5], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=Ec, batched=True, device=DEV,
                     seed=5, auto_reset=True)
        env.t.fill_(193)                                       # the time limit fires inside the first window
        actor, critic = OL.networks(torch, N)
        onorm, rn = ObsNormalizer(N, 6, DEV), rnorm()
        st = RolloutStorage(env, Tc, actions=True)
        return env, actor, critic, st, PPOLearner(actor, critic, 0.99, epochs=2, obs_norm=onorm, reward_norm=rn), onorm, rn

    def one_window(env, actor, critic, st, learner, onorm, rn):
        OL.normalised_window(env, actor, st, onorm)
        return learner.train(st)

    a = setup()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = one_window(*a)                                   # window 1 eagerly: builds every buffer, the carry among them
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = one_window(*a)
    b = setup()
    keys = sorted(out)
    snap = lambda env, actor, critic, st, learner, onorm, rn, o: [t.clone() for t in
                                                                  [getattr(m, n) for m in (actor, critic) for n in OL.NAMES] +
                                                                  [learner.actor_opt.m1, learner.critic_opt.m1, st.reward, st.actions, learner._rn,
                                                                   learner.G, learner.adv, onorm.state, rn.state, rn.scale, rn.ret] +
                                                                  [o[k] for k in keys]]
    ref = []
    for _ in range(3):
        o2 = one_window(*b)
        ref.append(snap(*b, o2))
    torch.cuda.synchronize()
    assert int(b[3].done.sum()) >= 0 and bool(torch.isfinite(b[3].reward).all())
    for rep in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        got = snap(*a, out)
        for j, (p, q) in enumerate(zip(got, ref[rep])):
            assert torch.equal(p, q), (rep, j)
        assert float(a[6].count.sum()) == (rep + 1) * Tc * Ec * N
    assert float(a[6].var.max()) > 0 and float((a[6].scale - 1).abs().min()) > 0 and all(torch.isfinite(t).all() for t in got)
