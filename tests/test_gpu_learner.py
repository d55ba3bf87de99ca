"""GPU tests of the batched learner (csrc/learner.hip; SAC_agents.py:280-357, `SA2CAgents.train_NN`): HIP gradients,
clip + Adam and the whole update against the reference's recorded update (tests/golden/learner_n5.npz) and against the
float64 restatement of the contract (tests/learner_ref.py, torch autograd used as checker only)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests import helpers as H
from tests import learner_ref as R

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def fx():
    return dict(H.load("learner_n5.npz"))


def make_mlp(W, kind):
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    return BatchedMLP(*W, kind, {0: 0, 1: 1, 2: 2}[kind], device=DEV)


def split(torch, flat, mlp):
    from scalable_collision_avoidance_rl_amd.learner import unflatten
    v = unflatten(flat, mlp.n_agents, mlp.d_in, mlp.h1, mlp.h2, mlp.nout)
    return [v[n] for n in NAMES]


def assert_grads(got, ref, mag, what, factor=1e-5):
    for name, g, r, m in zip(NAMES, got, ref, mag):
        g, r, m = (t.double().cpu() if hasattr(t, "cpu") else t for t in (g, r, m))
        g, r, m = (np.asarray(t, np.float64) for t in (g, r, m))
        assert np.all(np.isfinite(g)), (what, name)
        bad = np.abs(g - r) > factor * m + 1e-30
        assert not bad.any(), f"{what} {name}: {bad.sum()} / {bad.size} outside, worst excess {np.max(np.abs(g - r) - factor * m):.3e}"


def episode(torch):
    x, reward, done, act, nbr = R.episode_window(dict(H.load("episode_n5.npz")))
    return x.to(DEV), reward.to(DEV), done.to(DEV), act.to(DEV), nbr.to(DEV)


def storage_of(x, reward, done, act, nbr):
    """The parts of a RolloutStorage the learner reads."""
    return SimpleNamespace(z_pre=x, reward=reward, done=done, actions=act, nbr_pre=nbr)


def initial(fx, kind):
    actor, critic = R.reference_weights(kind, 5, 6, int(fx["seed_agents"] if kind == "softmax" else fx["seed_gauss"]))
    if critic is None:
        critic = R.reference_weights("softmax", 5, 6, int(fx["seed_agents"]))[1]
    return actor, critic


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["critic", "softmax", "gaussian"])
def test_gradients_on_the_episode_match_the_reference(torch, fx, net):
    from scalable_collision_avoidance_rl_amd.learner import mlp_gradients
    x, reward, done, act, nbr = episode(torch)
    T = x.shape[0]
    actor, critic = initial(fx, "gaussian" if net == "gaussian" else "softmax")
    i = int(fx["rec"])
    G = R.returns(reward, done, 0.99).float()
    w = torch.as_tensor(fx["w"], dtype=torch.float32, device=DEV).reshape(T, 1, 5)
    if net == "critic":
        W, kind, p, kw = critic, 0, "c", dict(target=G)
    else:
        W, kind, p, kw = actor, (1 if net == "softmax" else 2), net[0], dict(act=act, weight=w)
    mlp = make_mlp(W, kind)
    g, loss = mlp_gradients(mlp, x, **kw)
    mag = R.magnitude_grads(kind, [t.to(DEV) for t in W], x.reshape(T, 5, 6), 1.0 / T if kind == 0 else 1.0,
                            **{k: v.reshape(T, 5, *v.shape[3:]) for k, v in kw.items()})
    assert_grads([t[i] for t in split(torch, g, mlp)], [fx[f"{p}_grad_{n}"] for n in NAMES], [m[i] for m in mag], net)
    if net == "critic":
        np.testing.assert_allclose(loss.cpu().numpy(), fx["c_loss"], rtol=1e-5)


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["softmax", "gaussian"])
def test_one_train_on_the_episode_gives_the_reference_update(torch, fx, kind):
    from scalable_collision_avoidance_rl_amd.learner import SA2CLearner
    x, reward, done, act, nbr = episode(torch)
    actor_w, critic_w = initial(fx, kind)
    k = 1 if kind == "softmax" else 2
    actor, critic = make_mlp(actor_w, k), make_mlp(critic_w, 0)
    learner = SA2CLearner(actor, critic, 0.99)
    out = learner.train(storage_of(x, reward, done, act, nbr))
    torch.cuda.synchronize()
    p, i, stride = kind[0], int(fx["rec"]), int(fx["w2_stride"])
    np.testing.assert_allclose(out["critic_loss"].cpu().numpy(), fx["c_loss"], rtol=1e-5)
    np.testing.assert_allclose(out["critic_grad_norm"].cpu().numpy(), fx["c_norm"], rtol=2e-5)
    np.testing.assert_allclose(out["actor_grad_norm"].cpu().numpy(), fx[f"{p}_norm"], rtol=2e-5)
    aref = fx[f"{p}_loss"]
    np.testing.assert_allclose(out["actor_loss"].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    # the baseline came from the post-update critic: w as the reference computed it
    np.testing.assert_allclose(learner.w[:, 0].cpu().numpy(), fx["w"], rtol=1e-5, atol=1e-5 * np.abs(fx["w"]).max())
    ref64 = R.sa2c_train(k, actor_w, critic_w, x.cpu(), reward.cpu(), done.cpu(), act.cpu(), nbr.cpu(), 0.99)
    for pre, mlp, grads in (("c", critic, ref64["critic_grad"]), (p, actor, ref64["actor_grad"])):
        for name, g in zip(NAMES, grads):
            got = getattr(mlp, name)[i].double().cpu().numpy().reshape(-1)
            g = g[i].numpy().reshape(-1)
            key = f"{pre}_post_{name}"
            if name == "w2":
                got, g, key = got[::stride], g[::stride], f"{pre}_post_w2_sub"
            ref = fx[key].reshape(-1)
            tol = np.where(np.abs(g) > 1e-4, 1e-6, 1e-3 + 1e-6)
            assert np.all(np.abs(got - ref) <= tol), (pre, name, np.max(np.abs(got - ref) - tol))
    if k == 2:
        assert torch.all(actor.w3[:, :200, 2:] == 0) and torch.all(actor.w3[:, 200:, :2] == 0)
    assert torch.equal(learner.critic_opt.steps.cpu(), torch.ones(5, dtype=torch.int32))


# 3 --------------------------------------------------------------------------------------------------------------------
def random_net(torch, gen, N, d_in, h1, h2, nout):
    u = lambda *s, fan: ((torch.rand(*s, generator=gen) * 2 - 1) / math.sqrt(fan))
    return [u(N, d_in, h1, fan=d_in), u(N, h1, fan=d_in), u(N, h1, h2, fan=h1), u(N, h2, fan=h1), u(N, h2, nout, fan=h2),
            u(N, nout, fan=h2)]


def random_rows(torch, gen, T, E, N, d_in, nout, kind):
    x = (torch.rand(T, E, N, d_in, generator=gen) * 2 - 1) * 3
    target = torch.randn(T, E, N, generator=gen) * 5
    weight = torch.randn(T, E, N, generator=gen)
    if kind == 1:
        a = torch.randint(0, nout, (T, E, N), generator=gen).double() * 2 * math.pi / nout
        act = torch.stack([a.cos(), a.sin()], -1).float()
    else:
        act = torch.randn(T, E, N, 2, generator=gen) * 0.7
    return x, target, act, weight


FUZZ = [  # N, E, T, d_in, h1, h2, kind, nout, rows_per_chunk
    (1, 1, 1, 6, 37, 129, 0, 1, None),
    (5, 7, 37, 15, 200, 200, 1, 16, 64),
    (5, 96, 37, 6, 129, 38, 2, 4, 1024),
    (64, 1, 200, 6, 300, 300, 1, 16, 128),
    (64, 7, 37, 45, 200, 200, 0, 1, None),
    (256, 1, 37, 6, 400, 400, 2, 4, None),
    (256, 7, 1, 15, 37, 65, 1, 8, 64),
    (1, 96, 200, 45, 300, 301, 0, 1, 4096),
]


@pytest.mark.parametrize("case", FUZZ, ids=[f"N{c[0]}E{c[1]}T{c[2]}d{c[3]}h{c[4]}x{c[5]}k{c[6]}" for c in FUZZ])
def test_gradients_shape_fuzz_against_float64_autograd(torch, case):
    from scalable_collision_avoidance_rl_amd.learner import mlp_gradients
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    gen = torch.Generator().manual_seed(sum((j + 1) * (c or 0) for j, c in enumerate(case)))
    W = random_net(torch, gen, N, d_in, h1, h2, nout)
    if kind == 2:
        W[4] = W[4] * R.structural_mask(2, W)
    x, target, act, weight = random_rows(torch, gen, T, E, N, d_in, nout, kind)
    x = R.clean_rows(W, x, gen)
    mlp = make_mlp(W, kind)
    kw = dict(target=target) if kind == 0 else dict(act=act, weight=weight)
    g, loss = mlp_gradients(mlp, x, rows_per_chunk=rc, **kw)
    scale = 1.0 / (T * E) if kind == 0 else 1.0 / E
    Wd = [t.to(DEV) for t in W]
    rows = lambda t: t.to(DEV).reshape(T * E, N, *t.shape[3:])
    kwr = {k: rows(v) for k, v in kw.items()}
    ref, lref = R.grads(kind, Wd, rows(x), scale, **kwr)
    mag = R.magnitude_grads(kind, Wd, rows(x), scale, **kwr)
    assert_grads(split(torch, g, mlp), ref, mag, str(case))
    lmag = (scale * R.row_losses(kind, R.forward([w.double() for w in Wd], rows(x).double())[2],
                                 **{k: v.double() for k, v in kwr.items()}).abs().sum(1))
    assert torch.all((loss.double() - lref).abs() <= 1e-5 * lmag + 1e-30), (loss, lref)


def test_train_with_an_episode_end_mid_window_matches_float64(torch):
    """Returns and advantage exponents restart at `done`; the whole update against the float64 restatement."""
    from scalable_collision_avoidance_rl_amd.learner import SA2CLearner
    N, E, T, d_in = 5, 7, 37, 6
    gen = torch.Generator().manual_seed(3)
    Wa, Wc = random_net(torch, gen, N, d_in, 64, 48, 16), random_net(torch, gen, N, d_in, 40, 33, 1)
    x, _, act, _ = random_rows(torch, gen, T, E, N, d_in, 16, 1)
    x = R.clean_rows(Wa, R.clean_rows(Wc, x, gen), gen)
    x = R.clean_rows(Wc, x, gen)
    reward = torch.randn(T, E, N, generator=gen)
    done = torch.zeros(T, E, dtype=torch.uint8)
    done[11, ::2] = 1; done[25, 1] = 1
    nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(-1, N, (T, E, N), generator=gen),
                       torch.randint(0, N, (T, E, N), generator=gen)], -1).int()
    actor, critic = make_mlp(Wa, 1), make_mlp(Wc, 0)
    learner = SA2CLearner(actor, critic, 0.97, lr_actor=3e-4, lr_critic=2e-3)
    d = lambda t: t.to(DEV)
    out = learner.train(storage_of(d(x), d(reward), d(done), d(act), d(nbr)))
    ref = R.sa2c_train(1, Wa, Wc, x, reward, done, act, nbr, 0.97, lr_actor=3e-4, lr_critic=2e-3)
    np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(out["critic_grad_norm"].cpu().numpy(), ref["critic_norm"].numpy(), rtol=1e-4)
    np.testing.assert_allclose(out["actor_grad_norm"].cpu().numpy(), ref["actor_norm"].numpy(), rtol=1e-4)
    np.testing.assert_allclose(learner.w.cpu().numpy(), ref["w"].numpy(), rtol=1e-4, atol=1e-4 * float(ref["w"].abs().max()))
    for mlp, post, lr in ((critic, ref["critic_post"], 2e-3), (actor, ref["actor_post"], 3e-4)):
        for name, p in zip(NAMES, post):
            assert torch.all((getattr(mlp, name).double().cpu() - p).abs() <= lr * 0.02 + 1e-6), name


# 4 --------------------------------------------------------------------------------------------------------------------
def test_gradients_are_deterministic_and_normalised_per_env(torch):
    from scalable_collision_avoidance_rl_amd.learner import mlp_gradients
    N, T, d_in, E = 8, 200, 6, 12
    gen = torch.Generator().manual_seed(5)
    W = random_net(torch, gen, N, d_in, 300, 300, 16)
    x, _, act, weight = random_rows(torch, gen, T, 1, N, d_in, 16, 1)
    x = R.clean_rows(W, x, gen)
    mlp = make_mlp(W, 1)
    g1 = mlp_gradients(mlp, x, act=act, weight=weight, rows_per_chunk=128)[0].clone()
    g2 = mlp_gradients(mlp, x, act=act, weight=weight, rows_per_chunk=128)[0].clone()
    assert torch.equal(g1, g2)
    rep = lambda t: t.expand(T, E, *t.shape[2:]).contiguous()
    gE = mlp_gradients(mlp, rep(x), act=rep(act), weight=rep(weight), rows_per_chunk=128)[0]
    scale = 1.0
    mag = R.magnitude_grads(1, [t.to(DEV) for t in W], x.reshape(T, N, d_in).to(DEV), scale,
                            act=act.reshape(T, N, 2).to(DEV), weight=weight.reshape(T, N).to(DEV))
    assert_grads(split(torch, gE, mlp), split(torch, g1, mlp), mag, "E copies", factor=2e-5)


# 5 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 2])
def test_clip_and_adam_match_torch_over_five_steps(torch, kind):
    from scalable_collision_avoidance_rl_amd.learner import BatchedAdam, unflatten
    N, d_in, h1, h2, nout = 6, 6, 40, 32, (1 if kind == 0 else 4)
    gen = torch.Generator().manual_seed(9)
    W = random_net(torch, gen, N, d_in, h1, h2, nout)
    mask = R.structural_mask(kind, W)
    W[4] = W[4] * mask
    mlp = make_mlp(W, kind)
    opt = BatchedAdam(mlp, lr=2e-3, max_norm=10.0)
    params = [[torch.nn.Parameter(w[i].clone().to(DEV)) for w in W] for i in range(N)]
    topt = [torch.optim.Adam(p, lr=2e-3) for p in params]
    scales = torch.tensor([0.01, 0.3, 1.0, 5.0, 30.0, 100.0])          # total norms below and above max_norm
    for step in range(5):
        g = [torch.randn(*w.shape, generator=gen) * scales.view(-1, *([1] * (w.dim() - 1))) / 30 for w in W]
        g[4] = g[4] * mask
        flat = torch.cat([t.reshape(-1) for t in g]).to(DEV)
        norms = opt.step(flat).clone()
        tn = []
        for i in range(N):
            for p, gg in zip(params[i], g):
                p.grad = gg[i].to(DEV).clone()
            tn.append(float(torch.nn.utils.clip_grad_norm_(params[i], max_norm=10.0)))
            topt[i].step()
        np.testing.assert_allclose(norms.cpu().numpy(), tn, rtol=1e-5)
        for j, name in enumerate(NAMES):
            got = getattr(mlp, name)
            want = torch.stack([params[i][j].detach() for i in range(N)])
            assert torch.allclose(got, want, rtol=0, atol=2e-6), (step, name, float((got - want).abs().max()))
    assert int(opt.steps.min()) == int(opt.steps.max()) == 5
    if kind == 2:
        assert torch.all(mlp.w3[mask.to(DEV) == 0] == 0)
        assert torch.all(unflatten(opt.m1, N, d_in, h1, h2, nout)["w3"][mask.to(DEV) == 0] == 0)


# 6 --------------------------------------------------------------------------------------------------------------------
N_RS, G_RS, E_RS, T_RS = 16, 10.0, 32, 12


def storage_weights(torch, N=N_RS, actor_hidden=(48, 48), critic_hidden=(32, 32), actor_kind="softmax"):
    """The seeded networks of `storage_parts` (CPU tensors; needs no GPU): ``(wa, wc)``, a softmax-16 actor -- or, with
    ``actor_kind="gaussian"``, a four-output actor with the block-diagonal layer 3 -- and a critic, on 6 inputs."""
    gp = torch.Generator().manual_seed(0)
    rw = lambda *s: (torch.rand(*s, generator=gp) * 2 - 1) * 0.2
    (a1, a2), (c1, c2), nout = actor_hidden, critic_hidden, {"softmax": 16, "gaussian": 4}[actor_kind]
    wa = [rw(N, 6, a1), rw(N, a1), rw(N, a1, a2), rw(N, a2), rw(N, a2, nout), rw(N, nout)]
    wc = [rw(N, 6, c1), rw(N, c1), rw(N, c1, c2), rw(N, c2), rw(N, c2, 1), rw(N, 1)]
    if actor_kind == "gaussian":
        wa[4] = wa[4] * R.structural_mask(2, wa)
    return wa, wc


def storage_parts(torch, seed_env=5, N=N_RS, E=E_RS, T=T_RS, t0=193, config="f32", actor_kind="softmax", actor_hidden=(48, 48),
                  critic_hidden=(32, 32)):
    """``(env, actor, critic, storage)``: a batched env (k_closest 2, auto_reset) whose clock starts at ``t0`` -- the time limit
    fires ``199 - t0`` steps into the first window --, the networks of `storage_weights` built with the policy configuration
    ``config`` (tests/helpers.py: POLICY_CONFIGS; actor AND critic), a real RolloutStorage of T steps."""
    from scalable_collision_avoidance_rl_amd import drones
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    wa, wc = storage_weights(torch, N, actor_hidden, critic_hidden, actor_kind)
    env = drones(N, 0, [G_RS, G_RS], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True,
                 device=DEV, seed=seed_env, auto_reset=True)
    env.t.fill_(t0)                                        # the time limit fires inside the first window
    k = {"softmax": 1, "gaussian": 2}[actor_kind]
    kw = H.policy_kw(config)
    actor, critic = BatchedMLP(*wa, k, k, device=DEV, seed=7, **kw), BatchedMLP(*wc, 0, 0, device=DEV, **kw)
    return env, actor, critic, RolloutStorage(env, T, actions=True)


def storage_setup(torch, seed_env=5, setup=None, **learner_kw):
    """A batched env whose episodes end inside the first window, a softmax-16 actor, a critic, a real RolloutStorage
    (``setup``: other keywords of `storage_parts`) and an `SA2CLearner` (``learner_kw``: its keywords)."""
    from scalable_collision_avoidance_rl_amd.learner import SA2CLearner
    env, actor, critic, st = storage_parts(torch, seed_env, **(setup or {}))
    return env, actor, critic, st, SA2CLearner(actor, critic, 0.99, **learner_kw)


def rollout_window(env, actor, st):
    st.begin()
    for t in range(st.T):
        actor.sample_action(env.z, env=env, act_out=st.actions[t])
        env.step(st.actions[t], into=(st, t))


def test_consecutive_trains_on_a_rollout_storage_match_float64(torch):
    """Four rollout windows into a real RolloutStorage, each followed by SA2CLearner.train: every update (returns and
    advantage with an episode end in the first window, gradients, norms, Adam with the state carried over from the earlier
    updates) against the float64 restatement chained with its own Adam state from the same pre-update weights."""
    env, actor, critic, st, learner = storage_setup(torch)
    T, E, N = T_RS, E_RS, N_RS
    state = None
    for window in range(4):
        rollout_window(env, actor, st)
        torch.cuda.synchronize()
        Wa = [getattr(actor, n).detach().cpu().clone() for n in NAMES]
        Wc = [getattr(critic, n).detach().cpu().clone() for n in NAMES]
        data = [t.cpu().clone() for t in (st.z_pre, st.reward, st.done, st.actions, st.nbr_pre)]
        out = learner.train(st)
        torch.cuda.synchronize()
        ref = R.sa2c_train(1, Wa, Wc, *data, 0.99, state=state)
        state = ref["state"]
        if window == 0:
            assert int(data[2].sum()) == E                 # every env ended an episode inside the window
        np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * float(ref["G"].abs().max()))
        np.testing.assert_allclose(learner.w.cpu().numpy(), ref["w"].numpy(), rtol=1e-4, atol=1e-5 * float(ref["w"].abs().max()))
        np.testing.assert_allclose(out["critic_loss"].cpu().numpy(), ref["critic_loss"].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["critic_grad_norm"].cpu().numpy(), ref["critic_norm"].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["actor_grad_norm"].cpu().numpy(), ref["actor_norm"].numpy(), rtol=1e-5)
        for opt, mlp, post, m2 in ((learner.critic_opt, critic, ref["critic_post"], ref["state"]["cm2"]),
                                   (learner.actor_opt, actor, ref["actor_post"], ref["state"]["am2"])):
            assert int(opt.steps.min()) == int(opt.steps.max()) == window + 1
            for name, p, v in zip(NAMES, post, m2):
                got = getattr(mlp, name).double().cpu()
                # tight where the element's gradient scale is not tiny against its tensor's, within 2 lr elsewhere
                sharp = v.sqrt() > 1e-3 * float(v.sqrt().max())
                tol = torch.where(sharp, torch.full_like(p, 1e-6 + 1e-3 * opt.lr), torch.full_like(p, 2 * opt.lr))
                assert torch.all((got - p).abs() <= tol), (window, name, float(((got - p).abs() - tol).max()))


# 7 --------------------------------------------------------------------------------------------------------------------
def test_rollout_window_and_train_in_one_graph(torch):
    """A storage window (policy -> step, T steps) and SA2CLearner.train captured in ONE graph: three replays equal the
    same sequence run eagerly, bit for bit, and the optimisers' step counters advance on the device."""
    env, actor, critic, st, learner = storage_setup(torch)

    def window(env, actor, st, learner):
        rollout_window(env, actor, st)
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
    env2, actor2, critic2, st2, learner2 = storage_setup(torch)
    snap = lambda a, c, l, o: [t.clone() for t in (a.w1, a.b1, a.w2, a.b2, a.w3, a.b3, c.w1, c.b1, c.w2, c.b2, c.w3, c.b3,
                                                   l.actor_opt.m1, l.actor_opt.m2, l.critic_opt.m1, l.critic_opt.m2,
                                                   st2.z_pre if l is learner2 else st.z_pre,
                                                   o["actor_loss"], o["critic_loss"], o["actor_grad_norm"], o["critic_grad_norm"])]
    ref = []
    for _ in range(4):
        o2 = window(env2, actor2, st2, learner2)
        ref.append(snap(actor2, critic2, learner2, o2))
    torch.cuda.synchronize()
    for rep in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        got = snap(actor, critic, learner, out)
        for j, (a, b) in enumerate(zip(got, ref[rep])):
            assert torch.equal(a, b), (rep, j)
        assert int(learner.actor_opt.steps.min()) == int(learner.critic_opt.steps.max()) == rep + 1
    assert all(torch.isfinite(t).all() for t in got)


# 8 --------------------------------------------------------------------------------------------------------------------
def test_one_train_at_c3_size(torch):
    """N = 64 agents x E = 4096 envs x T = 200 steps, softmax-16 actor and critic: completes, finite everything."""
    from scalable_collision_avoidance_rl_amd.learner import SA2CLearner
    N, E, T, d_in = 64, 4096, 200, 6
    gen = torch.Generator(device=DEV).manual_seed(1)
    cpu = torch.Generator().manual_seed(1)
    actor, critic = make_mlp(random_net(torch, cpu, N, d_in, 300, 300, 16), 1), make_mlp(random_net(torch, cpu, N, d_in, 200, 200, 1), 0)
    x = (torch.rand(T, E, N, d_in, device=DEV, generator=gen) * 2 - 1) * 3
    reward = torch.randn(T, E, N, device=DEV, generator=gen)
    done = torch.zeros(T, E, dtype=torch.uint8, device=DEV)
    done[-1] = 1; done[99, ::3] = 1
    a = torch.randint(0, 16, (T, E, N), device=DEV, generator=gen).float() * (2 * math.pi / 16)
    act = torch.stack([a.cos(), a.sin()], -1)
    nbr = torch.stack([torch.arange(N, device=DEV).expand(T, E, N), torch.randint(0, N, (T, E, N), device=DEV, generator=gen),
                       torch.randint(-1, N, (T, E, N), device=DEV, generator=gen)], -1).int()
    learner = SA2CLearner(actor, critic, 0.99)
    out = learner.train(storage_of(x, reward, done, act, nbr))
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
    assert torch.isfinite(learner._actor_grad.grad).all() and torch.isfinite(learner._critic_grad.grad).all()
    assert float(out["critic_grad_norm"].min()) > 0 and float(out["actor_grad_norm"].min()) > 0
    for mlp in (actor, critic):
        assert all(torch.isfinite(getattr(mlp, n)).all() for n in NAMES)
