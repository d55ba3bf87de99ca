"""GPU tests of the PPO learner (csrc/learner.hip: the PPO head and the forward-only log-probability pass; csrc/dronesim.hip:
the neighbour advantage; `learner.PPOLearner`; SAC_agents.py:410-573, `SPPOAgents.train`) against the float64 restatement
of the contract (tests/ppo_ref.py) and the reference's own probabilities (tests/golden/ppo_n5.npz)."""
import math
import time

import numpy as np
import pytest

from tests import helpers as H
from tests import learner_ref as R
from tests import ppo_ref as P
from tests import test_gpu_learner as TG

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = TG.DEV
ACTOR_CASES = [c for c in TG.FUZZ if c[6] != 0]
SA2C_SECONDS = 1.88           # one SA2CLearner.train at C3 size on record (profiles/learner_lbench.jsonl)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def fx():
    return dict(H.load("learner_n5.npz"))


def weights_of(mlp):
    return [getattr(mlp, n).detach().cpu().clone() for n in NAMES]


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["softmax", "gaussian"])
def test_one_epoch_on_the_episode_has_ratio_one_and_gives_the_restated_update(torch, fx, kind):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    x, reward, done, act, nbr = TG.episode(torch)
    T = x.shape[0]
    actor_w, critic_w = TG.initial(fx, kind)
    k = 1 if kind == "softmax" else 2
    actor, critic = TG.make_mlp(actor_w, k), TG.make_mlp(critic_w, 0)
    learner = PPOLearner(actor, critic, 0.99, epochs=1)
    out = learner.train(TG.storage_of(x, reward, done, act, nbr))
    torch.cuda.synchronize()
    assert all(v.shape == (1, 5) for v in out.values())
    one = torch.ones(1, 5, device=DEV)
    assert torch.equal(out["ratio_min"], one) and torch.equal(out["ratio_max"], one)
    assert torch.equal(out["clip_fraction"], 0 * one) and torch.equal(out["approx_kl"], 0 * one)
    ref = P.ppo_train(k, actor_w, critic_w, x.cpu(), reward.cpu(), done.cpu(), act.cpu(), nbr.cpu(), 0.99, epochs=1)
    if k == 2:
        gold = dict(H.load("ppo_n5.npz"))
        np.testing.assert_allclose(torch.exp(learner.logp_old[:, 0]).cpu().numpy(), gold["p_old"], rtol=1e-5)
    np.testing.assert_allclose(learner.logp_old.cpu().numpy(), ref["logp_old"].numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(learner.adv.cpu().numpy(), ref["adv"].numpy(), rtol=1e-5, atol=1e-5 * float(ref["adv"].abs().max()))
    # the gradient buffer holds the CLIPPED gradient after the Adam step: scale the reference alike
    a = ref["actor"][0]
    coef = torch.clamp(10.0 / (ref["actor_norm"][0] + 1e-6), max=1.0)
    sc = lambda t: t * coef.view(-1, *([1] * (t.dim() - 1)))
    print(kind, "actor norm", ref["actor_norm"][0].numpy(), "loss", a["loss"].numpy())
    TG.assert_grads(TG.split(torch, learner._actor_grad.grad, actor), [sc(g) for g in a["grad"]], [sc(m) for m in a["mag"]], kind)
    np.testing.assert_allclose(out["critic_loss"][0].cpu().numpy(), ref["critic_loss"][0].numpy(), rtol=1e-5)
    np.testing.assert_allclose(out["critic_grad_norm"][0].cpu().numpy(), ref["critic_norm"][0].numpy(), rtol=2e-5)
    np.testing.assert_allclose(out["actor_grad_norm"][0].cpu().numpy(), ref["actor_norm"][0].numpy(), rtol=2e-5)
    aref = a["loss"].numpy()
    np.testing.assert_allclose(out["actor_loss"][0].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    assert torch.equal(learner.actor_opt.steps.cpu(), torch.ones(5, dtype=torch.int32))
    # the critic step is SA2CLearner's critic step: same weights, bit for bit
    actor2, critic2 = TG.make_mlp(actor_w, k), TG.make_mlp(critic_w, 0)
    out2 = SA2CLearner(actor2, critic2, 0.99).train(TG.storage_of(x, reward, done, act, nbr))
    torch.cuda.synchronize()
    for n in NAMES:
        assert torch.equal(getattr(critic, n), getattr(critic2, n)), n
    assert torch.equal(out["critic_loss"][0], out2["critic_loss"]) and torch.equal(out["critic_grad_norm"][0], out2["critic_grad_norm"])


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ACTOR_CASES, ids=[f"N{c[0]}E{c[1]}T{c[2]}d{c[3]}h{c[4]}x{c[5]}k{c[6]}" for c in ACTOR_CASES])
def test_ppo_head_away_from_ratio_one_matches_float64(torch, case):
    """`dronesim_mlp_grad_ppo` with a supplied logp_old: ratios over roughly [0.5, 2], advantages of both signs, ragged R,
    several chunks.  Rows within 1e-4 (relative) of a clip edge were redrawn by `ppo_ref.draw_logp_old`: at most 1 %."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    c = P.head_case(case)
    assert c["redrawn"] <= 0.01, c["redrawn"]
    rows = T * E
    mlp = TG.make_mlp(c["W"], kind)
    d = lambda t: t.to(DEV).contiguous()
    runner = GradientRunner(mlp, rows, rc)
    g, loss, stats = runner.run_ppo(d(c["x"]), 1.0 / rows, d(c["act"]), d(c["logp_old"]), d(c["adv"]), 0.2)
    torch.cuda.synchronize()
    r2 = lambda t: d(t).reshape(rows, N, *t.shape[3:])
    ref = P.actor_grads(kind, [d(w) for w in c["W"]], r2(c["x"]), r2(c["act"]), r2(c["logp_old"]), r2(c["adv"]), 0.2)
    assert not ref["near"].any()
    print(case, "redrawn", c["redrawn"], "clipped share", float(ref["clipped"].double().mean()),
          "r in", float(ref["r"].min()), float(ref["r"].max()))
    TG.assert_grads(TG.split(torch, g, mlp), ref["grad"], ref["mag"], str(case))
    count = torch.round(stats[0].double() * rows).long()
    assert torch.equal(count, ref["clipped"].sum(0)), (count, ref["clipped"].sum(0))
    np.testing.assert_allclose(stats[0].cpu().numpy(), ref["clip_fraction"].cpu().numpy(), rtol=1e-6)
    A = r2(c["adv"]).double()
    lmag = (ref["r"] * A).abs().sum(0) / rows
    assert torch.all((loss.double() - ref["loss"]).abs() <= 1e-5 * lmag + 1e-30), (loss, ref["loss"])
    klmag = (r2(c["logp_old"]).double().abs() + ref["logp"].abs()).mean(0)
    assert torch.all((stats[1].double() - ref["approx_kl"]).abs() <= 1e-5 * klmag), (stats[1], ref["approx_kl"])
    # a log-probability of magnitude |logp| carries 1e-5 |logp| of rounding into the ratio's exponent
    rtol = 1e-5 * (1 + float(ref["logp"].abs().max()))
    np.testing.assert_allclose(stats[2].cpu().numpy(), ref["ratio_min"].cpu().numpy(), rtol=rtol)
    np.testing.assert_allclose(stats[3].cpu().numpy(), ref["ratio_max"].cpu().numpy(), rtol=rtol)


def test_logp_pass_matches_float64_and_the_head_bit_for_bit(torch):
    """`dronesim_mlp_logp` against float64, and fed back as logp_old: every ratio exactly 1 whatever the chunking."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    for case in ACTOR_CASES[:3]:
        N, E, T, d_in, h1, h2, kind, nout, rc = case
        c = P.head_case(case)
        rows = T * E
        mlp = TG.make_mlp(c["W"], kind)
        d = lambda t: t.to(DEV).contiguous()
        runner = GradientRunner(mlp, rows, rc)
        lp = runner.logp(d(c["x"]), d(c["act"]), torch.empty(T, E, N, device=DEV))
        ref = P.logp(kind, [d(w) for w in c["W"]], d(c["x"]).reshape(rows, N, d_in), d(c["act"]).reshape(rows, N, 2))
        np.testing.assert_allclose(lp.reshape(rows, N).cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-5)
        _, _, stats = runner.run_ppo(d(c["x"]), 1.0 / rows, d(c["act"]), lp, d(c["adv"]), 0.2)
        one = torch.ones(N, device=DEV)
        assert torch.equal(stats[2], one) and torch.equal(stats[3], one)
        assert torch.equal(stats[0], 0 * one) and torch.equal(stats[1], 0 * one)


# 3 --------------------------------------------------------------------------------------------------------------------
N_RS, G_RS, E_RS, T_RS = TG.N_RS, TG.G_RS, TG.E_RS, TG.T_RS


def storage_setup(torch, seed_env=5, setup=None, **kw):
    """`test_gpu_learner.storage_setup` with a `PPOLearner` (``kw``: its keywords): a batched env whose episodes end inside the
    first window, a softmax-16 actor, a critic, a real RolloutStorage (``setup``: keywords of `test_gpu_learner.storage_parts`)."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    env, actor, critic, st = TG.storage_parts(torch, seed_env, **(setup or {}))
    return env, actor, critic, st, PPOLearner(actor, critic, 0.99, **kw)


@pytest.mark.parametrize("baseline", ["once", "per_neighbour"])
def test_four_epochs_on_a_rollout_storage_match_float64(torch, baseline):
    """One rollout window with an episode end inside it, then `PPOLearner.train(epochs=4)`: G, Q, Adv, and every epoch's
    losses, norms and clipped-row count, and the post-update weights, against the float64 restatement chained with its own
    Adam state from the same pre-update weights."""
    epochs = 4
    env, actor, critic, st, learner = storage_setup(torch, epochs=epochs, baseline=baseline)
    T, E, N = T_RS, E_RS, N_RS
    TG.rollout_window(env, actor, st)
    torch.cuda.synchronize()
    Wa, Wc = weights_of(actor), weights_of(critic)
    data = [t.cpu().clone() for t in (st.z_pre, st.reward, st.done, st.actions, st.nbr_pre)]
    assert int(data[2].sum()) == E                         # every env ended an episode inside the window
    out = learner.train(st)
    torch.cuda.synchronize()
    ref = P.ppo_train(1, Wa, Wc, *data, 0.99, epochs=epochs, baseline=baseline)
    amax = lambda t: float(t.abs().max())
    np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["G"]))
    np.testing.assert_allclose(learner.adv.cpu().numpy(), ref["adv"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["adv"]))
    c = 1.0 if baseline == "once" else (data[4] >= 0).sum(-1).to(DEV)
    Q = learner.adv + c * learner.V.view(T, E, N)
    np.testing.assert_allclose(Q.cpu().numpy(), ref["Q"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["Q"]))
    rows = T * E
    for ep in range(epochs):
        a = ref["actor"][ep]
        near = a["near"].sum(0)
        count = torch.round(out["clip_fraction"][ep].double().cpu() * rows).long()
        print(baseline, "epoch", ep, "clipped", count.tolist(), "ref", a["clipped"].sum(0).tolist(), "near an edge", near.tolist(),
              "r in", float(a["r"].min()), float(a["r"].max()))
        assert torch.all((count - a["clipped"].sum(0)).abs() <= near), (ep, count, a["clipped"].sum(0), near)
        np.testing.assert_allclose(out["critic_loss"][ep].cpu().numpy(), ref["critic_loss"][ep].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["critic_grad_norm"][ep].cpu().numpy(), ref["critic_norm"][ep].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["actor_grad_norm"][ep].cpu().numpy(), ref["actor_norm"][ep].numpy(), rtol=1e-5)
        aref = a["loss"].numpy()
        np.testing.assert_allclose(out["actor_loss"][ep].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    assert torch.equal(out["ratio_min"][0], torch.ones(N, device=DEV)) and torch.equal(out["ratio_max"][0], torch.ones(N, device=DEV))
    for opt, mlp, post, m2 in ((learner.critic_opt, critic, ref["critic_post"], ref["state"]["cm2"]),
                               (learner.actor_opt, actor, ref["actor_post"], ref["state"]["am2"])):
        assert int(opt.steps.min()) == int(opt.steps.max()) == epochs
        for name, p, v in zip(NAMES, post, m2):
            got = getattr(mlp, name).double().cpu()
            # per step taken: tight where the element's gradient scale is not tiny against its tensor's, within 2 lr elsewhere
            sharp = v.sqrt() > 1e-3 * float(v.sqrt().max())
            tol = epochs * torch.where(sharp, torch.full_like(p, 1e-6 + 1e-3 * opt.lr), torch.full_like(p, 2 * opt.lr))
            assert torch.all((got - p).abs() <= tol), (name, float(((got - p).abs() - tol).max()))


# 4 --------------------------------------------------------------------------------------------------------------------
def test_two_learners_on_the_same_data_are_bit_identical(torch):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    N, E, T, d_in = 6, 9, 41, 6
    gen = torch.Generator().manual_seed(17)
    Wa, Wc = TG.random_net(torch, gen, N, d_in, 72, 40, 4), TG.random_net(torch, gen, N, d_in, 40, 33, 1)
    Wa[4] = Wa[4] * R.structural_mask(2, Wa)
    x, _, act, _ = TG.random_rows(torch, gen, T, E, N, d_in, 4, 2)
    reward = torch.randn(T, E, N, generator=gen)
    done = torch.zeros(T, E, dtype=torch.uint8)
    done[20, ::2] = 1
    nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(-1, N, (T, E, N), generator=gen),
                       torch.randint(0, N, (T, E, N), generator=gen)], -1).int()
    d = lambda t: t.to(DEV).contiguous()
    runs = []
    for _ in range(2):
        actor, critic = TG.make_mlp(Wa, 2), TG.make_mlp(Wc, 0)
        learner = PPOLearner(actor, critic, 0.97, epochs=3, rows_per_chunk=128, lr_actor=3e-3)
        out = learner.train(TG.storage_of(d(x), d(reward), d(done), d(act), d(nbr)))
        torch.cuda.synchronize()
        runs.append([getattr(m, n).clone() for m in (actor, critic) for n in NAMES] +
                    [learner.actor_opt.m1, learner.actor_opt.m2, learner.critic_opt.m1, learner.critic_opt.m2, learner.adv,
                     learner.logp_old] + [out[k].clone() for k in sorted(out)])
    for j, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), j
    assert all(torch.isfinite(t).all() for t in runs[0])
    assert float(runs[0][-1].max()) >= 0                   # (the outputs are populated)


# 5 --------------------------------------------------------------------------------------------------------------------
def test_rollout_window_and_ppo_train_in_one_graph(torch):
    """A storage window (policy -> step, T steps) and PPOLearner.train (3 epochs) captured in ONE graph: three replays
    equal the same sequence run eagerly, bit for bit, and the step counters advance by 3 per replay on the device."""
    epochs = 3
    env, actor, critic, st, learner = storage_setup(torch, epochs=epochs)

    def window(env, actor, st, learner):
        TG.rollout_window(env, actor, st)
        return learner.train(st)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = window(env, actor, st, learner)              # window 1 eagerly: builds the slots and the learner's buffers
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = window(env, actor, st, learner)
    env2, actor2, critic2, st2, learner2 = storage_setup(torch, epochs=epochs)
    keys = sorted(out)
    snap = lambda a, c, l, s_, o: [t.clone() for t in [getattr(m, n) for m in (a, c) for n in NAMES] +
                                   [l.actor_opt.m1, l.actor_opt.m2, l.critic_opt.m1, l.critic_opt.m2, s_.z_pre, l.logp_old, l.adv] +
                                   [o[k] for k in keys]]
    ref = []
    for _ in range(4):
        o2 = window(env2, actor2, st2, learner2)
        ref.append(snap(actor2, critic2, learner2, st2, o2))
    torch.cuda.synchronize()
    for rep in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        got = snap(actor, critic, learner, st, out)
        for j, (a, b) in enumerate(zip(got, ref[rep])):
            assert torch.equal(a, b), (rep, j)
        assert int(learner.actor_opt.steps.min()) == int(learner.critic_opt.steps.max()) == epochs * (rep + 1)
    assert all(torch.isfinite(t).all() for t in got)


# 6 --------------------------------------------------------------------------------------------------------------------
def test_one_train_at_c3_size(torch):
    """N = 64 agents x E = 4096 envs x T = 200 steps, softmax-16 actor and critic, two epochs: completes within the time
    limit, finite everything, ratio exactly 1 in epoch 1.  The limit: an epoch launches a subset of one SA2CLearner.train
    (1.88 s on record at this size), the once-per-window part (one forward of each network) is less than another; twice that
    for the first call's allocations and a shared machine."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    N, E, T, d_in, epochs = 64, 4096, 200, 6, 2
    limit = 2 * (epochs + 1) * SA2C_SECONDS
    gen = torch.Generator(device=DEV).manual_seed(1)
    cpu = torch.Generator().manual_seed(1)
    actor = TG.make_mlp(TG.random_net(torch, cpu, N, d_in, 300, 300, 16), 1)
    critic = TG.make_mlp(TG.random_net(torch, cpu, N, d_in, 200, 200, 1), 0)
    x = (torch.rand(T, E, N, d_in, device=DEV, generator=gen) * 2 - 1) * 3
    reward = torch.randn(T, E, N, device=DEV, generator=gen)
    done = torch.zeros(T, E, dtype=torch.uint8, device=DEV)
    done[-1] = 1; done[99, ::3] = 1
    a = torch.randint(0, 16, (T, E, N), device=DEV, generator=gen).float() * (2 * math.pi / 16)
    act = torch.stack([a.cos(), a.sin()], -1)
    nbr = torch.stack([torch.arange(N, device=DEV).expand(T, E, N), torch.randint(0, N, (T, E, N), device=DEV, generator=gen),
                       torch.randint(-1, N, (T, E, N), device=DEV, generator=gen)], -1).int()
    learner = PPOLearner(actor, critic, 0.99, epochs=epochs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = learner.train(TG.storage_of(x, reward, done, act, nbr))
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"C3 PPO train, {epochs} epochs: {seconds:.2f} s (limit {limit:.2f} s)")
    assert seconds <= limit, (seconds, limit)
    for k, v in out.items():
        assert v.shape == (epochs, N) and torch.isfinite(v).all(), k
    assert torch.isfinite(learner._actor_grad.grad).all() and torch.isfinite(learner._critic_grad.grad).all()
    assert float(out["critic_grad_norm"].min()) > 0 and float(out["actor_grad_norm"].min()) > 0
    one = torch.ones(N, device=DEV)
    assert torch.equal(out["ratio_min"][0], one) and torch.equal(out["ratio_max"][0], one)
    assert float(out["clip_fraction"][0].max()) == 0.0
    assert float(out["clip_fraction"][1].min()) >= 0.0 and float(out["clip_fraction"][1].max()) <= 1.0
    assert float(out["ratio_min"][1].min()) > 0 and float(out["ratio_max"][1].max()) > float(out["ratio_min"][1].min())
    for mlp in (actor, critic):
        assert all(torch.isfinite(getattr(mlp, n)).all() for n in NAMES)


# 7 --------------------------------------------------------------------------------------------------------------------
def test_mlp_gradients_keep_their_bits_around_a_ppo_run(torch):
    """The shared GEMM / head code path is not disturbed: `mlp_gradients` on a fixed seeded input gives the same bits before
    and after a PPOLearner has run in the process (softmax, Gaussian and critic heads)."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, mlp_gradients
    N, E, T, d_in = 7, 5, 37, 6
    gen = torch.Generator().manual_seed(23)
    nets = {1: TG.random_net(torch, gen, N, d_in, 65, 40, 16), 2: TG.random_net(torch, gen, N, d_in, 40, 38, 4),
            0: TG.random_net(torch, gen, N, d_in, 33, 47, 1)}
    nets[2][4] = nets[2][4] * R.structural_mask(2, nets[2])
    inputs = {k: TG.random_rows(torch, gen, T, E, N, d_in, nets[k][5].shape[1], k) for k in nets}

    def all_grads():
        res = []
        for k, W in nets.items():
            x, target, act, weight = inputs[k]
            kw = dict(target=target) if k == 0 else dict(act=act, weight=weight)
            g, loss = mlp_gradients(TG.make_mlp(W, k), x, rows_per_chunk=64, **kw)
            res += [g.clone(), loss.clone()]
        return res

    before = all_grads()
    for k in (1, 2):
        x, _, act, _ = inputs[k]
        reward, done = torch.randn(T, E, N, generator=gen), torch.zeros(T, E, dtype=torch.uint8)
        nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N)] * 3, -1).int()
        d = lambda t: t.to(DEV).contiguous()
        learner = PPOLearner(TG.make_mlp(nets[k], k), TG.make_mlp(nets[0], 0), 0.99, epochs=2, rows_per_chunk=64)
        learner.train(TG.storage_of(d(x), d(reward), d(done), d(act), d(nbr)))
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(before, all_grads())):
        assert torch.equal(a, b), j
