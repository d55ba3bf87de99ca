"""GPU tests of parameter sharing across agent groups (csrc/learner.hip: dronesim_adam_step_shared, dronesim_kl_gate_shared,
dronesim_mlp_tie; `BatchedAdam(share=)`, `SA2CLearner(share=)`, `PPOLearner(share=)`, `BatchedMLP.tie_weights` / `take`): the
shared step bit for bit against the existing unshared step on the host's float64 group mean, a map of singletons against
``share=None``, tied training against the float64 restatement (tests/share_ref.py) with the bars of tests/test_gpu_learner.py and
tests/test_gpu_ppo_guard.py for the same quantities unshared, the group gate, capture, and the two `BatchedMLP` methods."""
import math

import numpy as np
import pytest

from tests import learner_ref as R
from tests import share_ref as S
from tests import test_gpu_learner as TG

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = "cuda:0"
MAP = [0, 1, 0, 2, 1, 0]
N, D_IN, H1, H2, T, E = 6, 6, 40, 32, 8, 16
KINDS = {1: 0, 4: 2, 16: 1}                      # nout -> out_kind: critic, Gaussian actor, softmax-16 actor


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def tied(torch, W, share):
    """The networks W [N, ...] with every member's tensors replaced by its leader's (on the host)."""
    group_of, groups = S.groups_of(share, W[0].shape[0])
    lead = S.leaders(groups)[torch.tensor(group_of)]
    return [w[lead].clone() for w in W]


def make_mlp(W, kind, **kw):
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    return BatchedMLP(*W, kind, kind, device=DEV, **kw)


def bits(t):
    """int32 view: NaN norms compare by their bits."""
    import torch
    return t.contiguous().view(torch.int32)


# 1 --------------------------------------------------------------------------------------------------------------------
# the shapes of test_gpu_learner.py's Adam test, and the network of its FUZZ row (256, 7, 1, 15, 37, 65, 1, 8, 64): per-agent
# tensors of 555, 37, 2405, 65, 520 and 8 elements -- short last quads, and slices that start off a 16-byte boundary -- under
# network_index(5, 256): one group of 252 members behind four singletons
STEP_CASES = [(N, D_IN, H1, H2, 1, MAP), (N, D_IN, H1, H2, 4, MAP), (N, D_IN, H1, H2, 16, MAP), (256, 15, 37, 65, 8, "index5")]


def step_inputs(torch, case):
    n, d_in, h1, h2, nout, share = case
    if share == "index5":
        from scalable_collision_avoidance_rl_amd.evaluate import network_index
        share = network_index(5, n)
    kind = KINDS.get(nout, 1)
    gen = torch.Generator().manual_seed(100 + nout + n)
    W = tied(torch, TG.random_net(torch, gen, n, d_in, h1, h2, nout), share)
    mask = R.structural_mask(kind, W)
    W[4] = W[4] * mask
    scales = 10.0 ** (torch.arange(n) % 6 - 3).float()                  # group norms below and above max_norm
    grads = []
    for _ in range(3):
        g = [torch.randn(*w.shape, generator=gen) * scales.view(-1, *([1] * (w.dim() - 1))) for w in W]
        g[4] = g[4] * mask
        grads.append(g)
    return share, kind, W, grads


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("case", STEP_CASES, ids=[f"N{c[0]}d{c[1]}h{c[2]}x{c[3]}o{c[4]}" for c in STEP_CASES])
def test_shared_step_is_the_unshared_step_on_the_float64_group_mean_bit_for_bit(torch, case, gated):
    """Three consecutive steps.  Reference: the host's group mean (float64, ascending members, one rounding) written into every
    member's slice, then the EXISTING dronesim_adam_step(_gated) on a copy of the tied network.  The shared step gets the raw
    gradients.  Every member's weights, the leaders' moments, all counters and all norms: equal bits.  Gated: one whole group
    is stopped -- unchanged, NaN norms."""
    from scalable_collision_avoidance_rl_amd.learner import BatchedAdam, unflatten
    share, kind, W, grads = step_inputs(torch, case)
    n = case[0]
    group_of, groups = S.groups_of(share, n)
    of, lead = torch.tensor(group_of), S.leaders(groups)
    ref_mlp, mlp = make_mlp(W, kind), make_mlp(W, kind)
    ref_opt, opt = BatchedAdam(ref_mlp, lr=2e-3, max_norm=10.0), BatchedAdam(mlp, lr=2e-3, max_norm=10.0, share=share)
    active = None
    if gated:
        stopped = 1                                                     # (a group of two under MAP, a singleton under index5)
        active = torch.tensor([0 if group_of[i] == stopped else 1 for i in range(n)], dtype=torch.int32, device=DEV)
    dims = (n,) + case[1:5]
    for step, g in enumerate(grads):
        mean = [S.group_mean_f32(t, groups)[of] for t in g]
        raw = torch.cat([t.reshape(-1) for t in g]).to(DEV)
        ref_flat = torch.cat([t.reshape(-1) for t in mean]).to(DEV)
        keep = raw.clone()
        ref_norm = ref_opt.step(ref_flat, active=active).clone()
        norm = opt.step(raw, active=active).clone()
        torch.cuda.synchronize()
        for name in NAMES:
            assert torch.equal(getattr(mlp, name), getattr(ref_mlp, name)), (step, name)
        # the leaders' slices are the live ones; a stopped group's gradient slice is left as it was (checked below), so the
        # clipped group gradient is compared on the leaders that stepped
        live = lead.to(DEV) if active is None else lead.to(DEV)[active[lead.to(DEV)] != 0]
        for buf, ref_buf, who in ((opt.m1, ref_opt.m1, lead.to(DEV)), (opt.m2, ref_opt.m2, lead.to(DEV)), (raw, ref_flat, live)):
            for name in NAMES:
                a, b = unflatten(buf, *dims)[name], unflatten(ref_buf, *dims)[name]
                assert torch.equal(a[who], b[who]), (step, name)
        assert torch.equal(opt.steps, ref_opt.steps) and torch.equal(bits(norm), bits(ref_norm)), step
        # the other members' slices of grad / m1 / m2 are left untouched
        others = torch.tensor([i for i in range(n) if i not in lead.tolist()], dtype=torch.long, device=DEV)
        for name in NAMES:
            assert torch.equal(unflatten(raw, *dims)[name][others], unflatten(keep, *dims)[name][others]), (step, name)
            assert not unflatten(opt.m1, *dims)[name][others].any() and not unflatten(opt.m2, *dims)[name][others].any()
        if gated:
            who = (active == 0)
            assert bool(torch.isnan(norm[who]).all()) and bool(torch.isfinite(norm[~who]).all())
            for name, w0 in zip(NAMES, W):
                assert torch.equal(getattr(mlp, name)[who], w0.to(DEV)[who]), name
            assert torch.equal(unflatten(raw, *dims)["w2"][who], unflatten(keep, *dims)["w2"][who])
            assert opt.steps[who].tolist() == [0] * int(who.sum())
    assert opt.steps[active != 0 if gated else slice(None)].tolist() == [3] * (n - (int((active == 0).sum()) if gated else 0))
    assert opt.share.tied(mlp)


# the learners' windows ------------------------------------------------------------------------------------------------
def window(torch, actor_nout, share, seed=3, spread=None):
    """A synthetic window of T = 8 steps x E = 16 envs for N = 6 agents: tied random networks (actor 6 -> 40 -> 32 -> nout, critic
    6 -> 40 -> 32 -> 1), rows away from the relu kinks of both, an episode end inside the window.  ``spread``: per-agent
    factors on the observations (agents whose policies move by different amounts).  CPU tensors."""
    kind = KINDS[actor_nout]
    gen = torch.Generator().manual_seed(seed)
    Wa = tied(torch, TG.random_net(torch, gen, N, D_IN, H1, H2, actor_nout), share)
    Wc = tied(torch, TG.random_net(torch, gen, N, D_IN, H1, H2, 1), share)
    if kind == 2:
        Wa[4] = Wa[4] * R.structural_mask(2, Wa)
    x, _, act, _ = TG.random_rows(torch, gen, T, E, N, D_IN, actor_nout, kind)
    scale = 3.0
    if spread is not None:
        x = x * torch.tensor(spread).view(1, 1, N, 1)
        scale = 3.0 * torch.tensor(spread).min().item()
    for _ in range(2):
        x = R.clean_rows(Wa, R.clean_rows(Wc, x, gen, scale=scale), gen, scale=scale)
    assert torch.equal(x, R.clean_rows(Wc, x, gen, scale=scale))
    reward = torch.randn(T, E, N, generator=gen)
    done = torch.zeros(T, E, dtype=torch.uint8)
    done[4, ::2] = 1
    nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(-1, N, (T, E, N), generator=gen),
                       torch.randint(0, N, (T, E, N), generator=gen)], -1).int()
    return kind, Wa, Wc, (x, reward, done, act, nbr)


def storage(data):
    return TG.storage_of(*[t.to(DEV).contiguous() for t in data])


def state_of(torch, learner, out):
    return ([getattr(m, n).clone() for m in (learner.actor, learner.critic) for n in NAMES] +
            [t.clone() for t in (learner.actor_opt.m1, learner.actor_opt.m2, learner.critic_opt.m1, learner.critic_opt.m2,
                                 learner.actor_opt.steps, learner.critic_opt.steps)] + [out[k].clone() for k in sorted(out)])


# 2 --------------------------------------------------------------------------------------------------------------------
def test_a_map_of_singletons_is_the_unshared_learner_bit_for_bit(torch):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    kind, Wa, Wc, data = window(torch, 4, None)
    runs = []
    for share in (list(range(N)), None):
        learner = PPOLearner(make_mlp(Wa, kind), make_mlp(Wc, 0), 0.97, epochs=2, minibatches=2, ent_coef=0.01, vf_clip=0.2,
                             target_kl=0.02, lr_actor=3e-3, share=share)
        out = learner.train(storage(data))
        torch.cuda.synchronize()
        runs.append((sorted(out), state_of(torch, learner, out)))
    assert runs[0][0] == runs[1][0]
    for j, (a, b) in enumerate(zip(runs[0][1], runs[1][1])):
        assert torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b), j
    assert all(bool(torch.isfinite(t).all()) for t in runs[0][1][:12])


# 3 --------------------------------------------------------------------------------------------------------------------
def assert_tied(torch, mlp, share, what):
    group_of, groups = S.groups_of(share, mlp.n_agents)
    lead = S.leaders(groups)[torch.tensor(group_of)].to(DEV)
    for name in NAMES:
        w = getattr(mlp, name)
        assert torch.equal(w, w[lead]), (what, name)
    gen = torch.Generator().manual_seed(5)
    z = ((torch.rand(33, 1, mlp.d_in, generator=gen) * 2 - 1) * 3).expand(33, mlp.n_agents, mlp.d_in).contiguous().to(DEV)
    out = mlp.forward(z)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, out[:, lead]), (what, "forward")


def assert_weights(torch, mlp, opt, post, m2, n_steps, what):
    """The bar of the unshared learners' tests per step taken: tight where the element's gradient scale is not tiny against its
    tensor's, within 2 lr elsewhere (a gradient at rounding level decides the sign of Adam's first steps)."""
    for name, p, v in zip(NAMES, post, m2):
        got = getattr(mlp, name).double().cpu()
        sharp = v.sqrt() > 1e-3 * float(v.sqrt().max())
        tol = n_steps * torch.where(sharp, torch.full_like(p, 1e-6 + 1e-3 * opt.lr), torch.full_like(p, 2 * opt.lr))
        assert torch.all((got - p).abs() <= tol), (what, name, float(((got - p).abs() - tol).max()))


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("share", ["all", MAP], ids=["all", "map"])
def test_sa2c_tied_training_matches_the_float64_restatement(torch, share, precision):
    from scalable_collision_avoidance_rl_amd.learner import SA2CLearner
    kind, Wa, Wc, data = window(torch, 16, share)
    actor, critic = make_mlp(Wa, kind, precision=precision), make_mlp(Wc, 0, precision=precision)
    learner = SA2CLearner(actor, critic, 0.97, lr_actor=3e-4, lr_critic=2e-3, share=share)
    out = learner.train(storage(data))
    torch.cuda.synchronize()
    for mlp, what in ((actor, "actor"), (critic, "critic")):
        assert_tied(torch, mlp, share, what)
    assert learner.actor_opt.steps.tolist() == [1] * N and learner.critic_opt.steps.tolist() == [1] * N
    if precision != "f32":
        return          # (the restatement's bars are those of the exact float32 forward)
    ref = S.sa2c_train(share, kind, Wa, Wc, *data, 0.97, lr_actor=3e-4, lr_critic=2e-3)
    np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * float(ref["G"].abs().max()))
    np.testing.assert_allclose(learner.w.cpu().numpy(), ref["w"].numpy(), rtol=1e-4, atol=1e-4 * float(ref["w"].abs().max()))
    np.testing.assert_allclose(out["critic_loss"].cpu().numpy(), ref["critic_loss"].numpy(), rtol=1e-5)
    np.testing.assert_allclose(out["critic_grad_norm"].cpu().numpy(), ref["critic_norm"].numpy(), rtol=1e-4)
    np.testing.assert_allclose(out["actor_grad_norm"].cpu().numpy(), ref["actor_norm"].numpy(), rtol=1e-4)
    aref = ref["actor_loss"].numpy()
    np.testing.assert_allclose(out["actor_loss"].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    assert_weights(torch, critic, learner.critic_opt, ref["critic_post"], ref["cm2"], 1, "critic")
    assert_weights(torch, actor, learner.actor_opt, ref["actor_post"], ref["am2"], 1, "actor")


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("share", ["all", MAP], ids=["all", "map"])
def test_ppo_tied_training_in_minibatches_matches_the_float64_restatement(torch, share, precision):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    epochs, K, seed = 2, 2, 2 ** 40 + 3
    kind, Wa, Wc, data = window(torch, 4, share)
    actor, critic = make_mlp(Wa, kind, precision=precision), make_mlp(Wc, 0, precision=precision)
    learner = PPOLearner(actor, critic, 0.97, epochs=epochs, minibatches=K, shuffle_seed=seed, lr_actor=3e-3, share=share)
    out = {k: v.clone() for k, v in learner.train(storage(data)).items()}
    torch.cuda.synchronize()
    for mlp, what in ((actor, "actor"), (critic, "critic")):
        assert_tied(torch, mlp, share, what)
    steps = epochs * K
    assert learner.actor_opt.steps.tolist() == [steps] * N and learner.critic_opt.steps.tolist() == [steps] * N
    if precision != "f32":
        return
    ref = S.ppo_train(share, kind, Wa, Wc, *data, 0.97, epochs=epochs, minibatches=K, shuffle_seed=seed, lr_actor=3e-3)
    assert np.array_equal(learner.perm.cpu().numpy(), ref["perms"][-1])
    amax = lambda t: float(t.abs().max())
    np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["G"]))
    np.testing.assert_allclose(learner.adv.cpu().numpy(), ref["adv"].numpy(), rtol=1e-4, atol=1e-4 * amax(ref["adv"]))
    M = T * E // K
    for ep in range(epochs):
        for b in range(K):
            j, a = ep * K + b, ref["actor"][ep * K + b]
            count = torch.round(out["clip_fraction"][ep, b].double().cpu() * M).long()
            near = a["near"].sum(0)
            print(share, "step", j, "clipped", count.tolist(), "ref", a["clipped"].sum(0).tolist(), "near", near.tolist())
            assert torch.all((count - a["clipped"].sum(0)).abs() <= near), (j, count, a["clipped"].sum(0), near)
            np.testing.assert_allclose(out["critic_loss"][ep, b].cpu().numpy(), ref["critic_loss"][j].numpy(), rtol=1e-5)
            np.testing.assert_allclose(out["critic_grad_norm"][ep, b].cpu().numpy(), ref["critic_norm"][j].numpy(), rtol=1e-5)
            np.testing.assert_allclose(out["actor_grad_norm"][ep, b].cpu().numpy(), ref["actor_norm"][j].numpy(), rtol=1e-5)
            aref = a["loss"].numpy()
            np.testing.assert_allclose(out["actor_loss"][ep, b].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    assert_weights(torch, critic, learner.critic_opt, ref["critic_post"], ref["cm2"], steps, "critic")
    assert_weights(torch, actor, learner.actor_opt, ref["actor_post"], ref["am2"], steps, "actor")


# 4 --------------------------------------------------------------------------------------------------------------------
GATE_EPOCHS, GATE_SEED, GATE_SPREAD = 4, 3, (0.2, 0.4, 0.7, 1.0, 1.0, 1.0)


def gate_case(torch):
    """The window of the gate test, its UNGATED restatement and the threshold: the geometric mean of the group's KL at the two
    consecutive steps around the stop."""
    kind, Wa, Wc, data = window(torch, 4, "all", seed=GATE_SEED, spread=GATE_SPREAD)
    kw = dict(epochs=GATE_EPOCHS, lr_actor=3e-3)
    free = S.ppo_train("all", kind, Wa, Wc, *data, 0.97, **kw)
    group = [float(k[0]) for k in free["group_kl"]]
    stop = 2                                                            # (step 0's KL is exactly 0: the window's own policy)
    tau = math.sqrt(group[stop - 1] * group[stop])
    return kind, Wa, Wc, data, kw, free, group, stop, tau


def test_the_group_gate_stops_on_the_mean_kl_of_the_members(torch):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    kind, Wa, Wc, data, kw, free, group, stop, tau = gate_case(torch)
    own = free["kl"][stop]
    print("group kl per step", group, "tau", tau, "members' own kl at the stop", own.tolist())
    # conditions on the inputs: a factor 2 between the two steps, the steps before the stop below the threshold, and a member
    # whose own estimate is on the other side at the stopping step (per-agent gating would let it go on)
    assert group[stop] >= 2 * group[stop - 1] > 0 and all(g <= tau for g in group[:stop])
    assert bool((own <= tau).any()) and bool((own > tau).any())
    ref = S.ppo_train("all", kind, Wa, Wc, *data, 0.97, target_kl=tau, **kw)
    assert ref["actor_steps"].tolist() == [stop] * N
    actor, critic = make_mlp(Wa, kind), make_mlp(Wc, 0)
    learner = PPOLearner(actor, critic, 0.97, target_kl=tau, share="all", **kw)
    out = learner.train(storage(data))
    torch.cuda.synchronize()
    assert out["actor_steps"].dtype == torch.int32 and out["actor_steps"].tolist() == [stop] * N
    assert learner.actor_opt.steps.tolist() == [stop] * N and learner.active.tolist() == [0] * N
    assert learner.critic_opt.steps.tolist() == [GATE_EPOCHS] * N       # the critics keep stepping
    assert_tied(torch, actor, "all", "actor")
    assert_tied(torch, critic, "all", "critic")
    kl = out["kl"].double().cpu()
    for ep in range(GATE_EPOCHS):
        computed, stepped = ep <= stop, ep < stop
        assert bool(torch.isfinite(out["actor_loss"][ep]).all()) == computed and bool(torch.isfinite(kl[ep]).all()) == computed, ep
        assert bool(torch.isfinite(out["actor_grad_norm"][ep]).all()) == stepped, ep
        if not computed:
            assert bool(torch.isnan(kl[ep]).all()) and bool(torch.isnan(out["actor_grad_norm"][ep]).all())
        if stepped:
            norms = out["actor_grad_norm"][ep]
            assert torch.equal(norms, norms[0].expand(N))               # the group's norm in every member's slot
            np.testing.assert_allclose(norms.cpu().numpy(), ref["actor_norm"][ep].numpy(), rtol=1e-5)
    assert float(kl[0].abs().max()) == 0.0
    # the members' own estimates are still per agent, and the device's group mean is on the restatement's side of the threshold
    assert float(kl[stop].min()) <= tau < float(kl[stop].max()) and float(kl[stop].mean()) > tau >= float(kl[stop - 1].mean())
    assert_weights(torch, actor, learner.actor_opt, ref["actor_post"], ref["am2"], stop, "actor")


# 5 --------------------------------------------------------------------------------------------------------------------
def test_a_captured_shared_train_replays_like_eager_calls(torch):
    """`train()` with ``share="all"`` (target_kl, minibatches) captured in a graph: after one eager call, two replays equal the
    second and third eager call of an identical learner, bit for bit, and the counters advance on the device."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    kind, Wa, Wc, data = window(torch, 4, "all")
    kw = dict(epochs=2, minibatches=2, target_kl=1e30, lr_actor=3e-3, share="all")
    learner = PPOLearner(make_mlp(Wa, kind), make_mlp(Wc, 0), 0.97, **kw)
    st = storage(data)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = learner.train(st)                                        # call 1 eagerly: builds the learner's buffers
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = learner.train(st)
    learner2 = PPOLearner(make_mlp(Wa, kind), make_mlp(Wc, 0), 0.97, **kw)
    st2 = storage(data)
    ref = []
    for _ in range(3):
        o2 = learner2.train(st2)
        torch.cuda.synchronize()
        ref.append(state_of(torch, learner2, o2))
    for rep in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        got = state_of(torch, learner, out)
        for j, (a, b) in enumerate(zip(got, ref[rep])):
            assert torch.equal(a, b), (rep, j)
        assert learner.actor_opt.steps.tolist() == [4 * (rep + 1)] * N
        assert_tied(torch, learner.actor, "all", "actor")
    assert all(bool(torch.isfinite(t).all()) for t in got)


# 6 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nout", [1, 16])
def test_tie_weights_makes_members_equal_their_leaders_and_lets_the_optimiser_construct(torch, nout):
    from scalable_collision_avoidance_rl_amd.learner import BatchedAdam
    kind = KINDS[nout]
    gen = torch.Generator().manual_seed(21)
    W = TG.random_net(torch, gen, N, D_IN, H1, H2, nout)
    mlp = make_mlp(W, kind)
    with pytest.raises(ValueError, match="tie_weights"):
        BatchedAdam(mlp, share=MAP)
    assert mlp.tie_weights(MAP) is mlp
    torch.cuda.synchronize()
    for name, w0 in zip(NAMES, tied(torch, W, MAP)):
        assert torch.equal(getattr(mlp, name), w0.to(DEV)), name
    assert_tied(torch, mlp, MAP, "tied")                               # (the forward images were refreshed)
    opt = BatchedAdam(mlp, share=MAP)
    assert opt.share.n_groups == 3 and opt.share.members.tolist() == [0, 2, 5, 1, 4, 3] and opt.share.group_ptr.tolist() == [0, 3, 5, 6]
    assert BatchedAdam(make_mlp(W, kind)).share is None


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_take_lays_networks_out_for_another_team(torch, precision):
    index = [0, 0, 2, 2, 2, 1, 0, 0]
    gen = torch.Generator().manual_seed(22)
    W = TG.random_net(torch, gen, N, D_IN, H1, H2, 16)
    src = make_mlp(W, 1, precision=precision, seed=9)
    dst = src.take(index)
    assert (dst.n_agents, dst.precision, dst.out_kind, dst.sample_kind, dst.seed, dst._mode) == (8, precision, 1, 1, 9, src._mode)
    rows = (torch.rand(19, 1, D_IN, generator=gen) * 2 - 1) * 3
    want = src.forward(rows.expand(19, N, D_IN).contiguous().to(DEV))
    got = dst.forward(rows.expand(19, 8, D_IN).contiguous().to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(got, want[:, torch.tensor(index, device=DEV)])
    for name, w0 in zip(NAMES, W):
        assert torch.equal(getattr(dst, name), w0[index].to(DEV)), name
    for bad in ([], [0, 6], [0, -1], [0, 1.0], [True, 0]):
        with pytest.raises(ValueError):
            src.take(bad)
