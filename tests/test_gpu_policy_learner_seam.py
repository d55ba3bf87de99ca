"""GPU tests of the seam between the acting kernels and the learner: the policy that acts is the policy the learner just updated.

The five policy-forward families (`BatchedMLP.forward` / `sample_action`) read PACKED snapshots of the weights (`BatchedMLP._packed`);
the learner (csrc/learner.hip) reads and writes the plain arrays ``w1 .. b3`` and re-packs the snapshots once per network per
``train()`` (`BatchedAdam.step(refresh=last)`, the gated actor step included).  Every other learner test takes a window's data as given,
so a missed re-pack, a wrong action index or an action stored against the wrong observation changes nothing it compares.  Here:

  images     after every ``train()`` of every learner path and policy configuration each image IS `_pack()` of the live weights, in the
             buffer the constructor made; the forward equals the float64 forward of the live weights and misses that of the weights
             before the update by >= 10 bars (tests/test_policy_learner_seam_host.py shows the update is that large)
  actions    every unit vector the sampler can emit, for nout = 1 .. 32, is read back by the learner as the index the sampler reports
  on-policy  in the window after an update, exp(logp_old) of the stored (observation, action) pairs is the probability the acting
             kernel gave that action when it sampled it; the Gaussian density likewise; PPO's V is the updated critic's

Shapes (tests/seam_ref.py): N = 5, T = 6, E = the configuration's row block + 1, hidden widths 48 / 40, an episode end in window 1."""
import time

import pytest

from tests import helpers as H
from tests import learner_ref as R
from tests import seam_ref as S
from tests import test_gpu_learner as TG
from tests import test_gpu_ppo as TP

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = TG.DEV
T, N = S.T, S.N
_T0 = time.perf_counter()


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield torch
    print(f"\ntests/test_gpu_policy_learner_seam.py: {time.perf_counter() - _T0:.1f} s since the module was imported")


def build(torch, config, kind, path):
    """``(env, actor, critic, storage, learner)`` of one (configuration, actor kind, learner path of `seam_ref.LEARNERS`)."""
    cls, kw = S.LEARNERS[path] if isinstance(path, str) else path
    setup = TG.storage_setup if cls == "SA2CLearner" else TP.storage_setup
    return setup(torch, setup=S.setup_of(config, kind), **kw)


def image_ptrs(mlp):
    return {name: t.data_ptr() for name, t in mlp._packed.items()}


def assert_images_are_the_live_weights(torch, mlp, ptrs, what):
    """Check 1: every image equals `_pack()` of the live weights bit for bit, at the address the constructor recorded."""
    fresh = mlp._pack()
    assert set(fresh) == set(mlp._packed) == set(ptrs), what
    for name, image in mlp._packed.items():
        assert image.data_ptr() == ptrs[name], (what, name, "the image moved")
        assert torch.equal(image, fresh[name]), (what, name, "the image is not the live weights'")


def assert_forward_is_the_live_weights(torch, mlp, kind, x, config, what, stale=None):
    """Check 2: `forward(x)` against the float64 forward of the live ``w1 .. b3`` at the configuration's bar; check 3 (``stale``: the
    weights before the update; the six float32-accurate configurations): against THEIR float64 forward every agent misses by >= 10 bars."""
    out = mlp.forward(x)
    live = S.misses(out, S.forward64(TP.weights_of(mlp), x, kind), config)
    print(what, "live weights: worst", f"{float(live.max()):.3f}", "bars", end="")
    assert torch.all(live <= 1.0), (what, live)
    if stale is not None and config != "bf16":
        old = S.misses(out, S.forward64(stale, x, kind), config)
        print("; weights before the update:", [f"{v:.0f}" for v in old.tolist()], "bars", end="")
        assert torch.all(old >= S.TEETH), (what, old)
    print()


def every_env_ended_an_episode(st):
    return bool(st.done.bool().any(0).all())


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("path", list(S.LEARNERS))
@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
def test_after_train_every_image_is_the_live_weights(torch, config, path, kind):
    """Two windows of rollout + ``train()``; after each, checks 1 - 3 above on actor and critic, both built with ``config``.  The probe
    rows are window 2's first observations (ring slot T of window 1, which window 2 must start from)."""
    env, actor, critic, st, learner = build(torch, config, kind, path)
    nets = (("actor", actor, kind), ("critic", critic, "critic"))
    ptrs = {what: image_ptrs(mlp) for what, mlp, _ in nets}
    assert all(bool(p) == (config != "f32-w2-unpacked") for p in ptrs.values())
    probe = None
    for window in (1, 2):
        TG.rollout_window(env, actor, st)
        if window == 2:
            assert torch.equal(st.z_pre[0], probe)
        before = {what: TP.weights_of(mlp) for what, mlp, _ in nets}
        out = learner.train(st)
        torch.cuda.synchronize()
        if window == 1:
            assert every_env_ended_an_episode(st)
            probe = st.z_all[T].clone()
        if path == "ppo-frozen":
            assert out["actor_steps"].tolist() == [1] * N
        if path == "ppo-guards":
            assert out["actor_steps"].tolist() == [S.LEARNERS[path][1]["epochs"]] * N
        for what, mlp, k in nets:
            tag = f"{config} {path} {kind} window {window} {what}:"
            assert_images_are_the_live_weights(torch, mlp, ptrs[what], tag)
            assert_forward_is_the_live_weights(torch, mlp, k, probe, config, tag, stale=before[what])


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("path", ["sa2c", ("PPOLearner", dict(epochs=2))], ids=["sa2c", "ppo-e2"])
@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
def test_images_follow_the_weights_inside_a_captured_window(torch, config, path, kind):
    """A rollout window and ``train()`` captured in ONE graph (as tests/test_gpu_ppo.py: test_rollout_window_and_ppo_train_in_one_graph),
    replayed twice: the re-pack -- for f16x2 with the power-of-two factors recomputed -- runs inside the graph, into the buffers the
    captured policy launches read, so it may do nothing a stream capture forbids (the split streams' packing once built its index table
    with a host-to-device copy on every call: hipErrorStreamCaptureUnsupported for bf16x3 and the f16x2 split kernel).  Checks 1 - 3
    after the last replay, and the weights did move in it."""
    env, actor, critic, st, learner = build(torch, config, kind, path)
    nets = (("actor", actor, kind), ("critic", critic, "critic"))
    ptrs = {what: image_ptrs(mlp) for what, mlp, _ in nets}

    def window():
        TG.rollout_window(env, actor, st)
        return learner.train(st)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        window()                                           # window 1 eagerly: builds the slots and the learner's buffers
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        window()
    graph.replay()
    torch.cuda.synchronize()
    before = {what: TP.weights_of(mlp) for what, mlp, _ in nets}
    graph.replay()
    torch.cuda.synchronize()
    probe = st.z_pre[0].clone()
    for what, mlp, k in nets:
        tag = f"{config} captured {kind} {what}:"
        assert any(not torch.equal(a, b) for a, b in zip(before[what], TP.weights_of(mlp))), tag
        assert_images_are_the_live_weights(torch, mlp, ptrs[what], tag)
        assert_forward_is_the_live_weights(torch, mlp, k, probe, config, tag, stale=before[what])


# 2 ---------------------------------------------------------------------------------------------------------------------
_PROBES = {}


def probe_actor(torch, nout):
    """The probe of one nout: ``nout`` agents on a 1-1-1 network of zero weights with b3[j] = -0.25 j for every agent -- log-probabilities
    0.25 apart, far above float32 error -- and its `GradientRunner` for the 3 rows (the learner reads the plain arrays: one probe serves
    every configuration).

    nout = 1 is a documented limit of the learner, not of the sampler -- include/dronesim.h on the learner's entry points: "out_kind 0
    with nout = 1, 1 with nout >= 2, 2 with nout = 4 and an even h2" -- so there the runner is None and the refusal is asserted."""
    if nout not in _PROBES:
        from scalable_collision_avoidance_rl_amd import _native
        from scalable_collision_avoidance_rl_amd.learner import GradientRunner
        from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
        z = lambda *s: torch.zeros(*s)
        b3 = (-0.25 * torch.arange(nout, dtype=torch.float32)).expand(nout, nout).contiguous()
        mlp = BatchedMLP(z(nout, 1, 1), z(nout, 1), z(nout, 1, 1), z(nout, 1), z(nout, 1, nout), b3, 1, 1, device=DEV)
        if nout == 1:
            with pytest.raises(_native.DroneSimError, match="1 nout >= 2") as refusal:
                GradientRunner(mlp, 3)
            assert refusal.value.code == _native.EINVAL
            runner = None
        else:
            runner = GradientRunner(mlp, 3)
        _PROBES[nout] = (mlp, runner, torch.log_softmax(b3[0].double(), -1))
    return _PROBES[nout]


@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
@pytest.mark.parametrize("nout", range(1, 33))
def test_every_action_the_sampler_emits_is_the_action_the_learner_reads(torch, nout, config):
    """A forcing policy -- agent j has b3[j] = 0 and -80 elsewhere, all weights zero -- makes the sampler of ``config`` emit its own unit
    vector (v_cos_f32 / v_sin_f32 of pick x an approximate 1 / nout) for EVERY index j.  The learner's `dronesim_mlp_logp` on the probe
    actor then returns log_softmax(b3)[idx] with idx the index the sampler reported, i.e. `action_of` (rintf(atan2f ...)) recovered exactly
    that index; so do the two float64 checkers.  A uniform draw of exactly 0 picks index 0 by the sampler's rule (the first j with
    u < cdf_j; e^-80 > 0): at most one such row per nout.  At nout = 1 the learner takes no softmax actor (`probe_actor`: the header's
    sentence); the sampler's side and the float64 checkers are still held to index 0 and the unit vector (1, 0)."""
    from scalable_collision_avoidance_rl_amd.learner import action_index
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    E = 3
    z = lambda *s: torch.zeros(*s)
    b3 = torch.full((nout, nout), -80.0)
    b3.fill_diagonal_(0.0)
    forcing = BatchedMLP(z(nout, 1, 1), z(nout, 1), z(nout, 1, 1), z(nout, 1), z(nout, 1, nout), b3, 1, 1, device=DEV, seed=nout,
                         **H.policy_kw(config))
    x = torch.zeros(E, nout, 1, device=DEV)
    idx = torch.full((E, nout), -1, dtype=torch.int32, device=DEV)
    act, idx2 = forcing.sample_action(x, return_outputs=False, idx_out=idx)
    assert idx2 is idx
    probe, runner, logsm = probe_actor(torch, nout)
    lp = None if runner is None else runner.logp(x, act, torch.empty(E, nout, device=DEV))
    torch.cuda.synchronize()
    idx, act = idx.cpu().long(), act.cpu()
    want = torch.arange(nout).expand(E, nout)
    zero_draws = int((idx != want).sum())
    print(f"nout {nout} {config}: rows off the forced index: {zero_draws}")
    assert zero_draws <= 1 and torch.all((idx == want) | (idx == 0))
    if runner is None:
        assert nout == 1 and torch.equal(act, torch.tensor([1.0, 0.0]).expand(E, 1, 2))
    else:
        lp = lp.cpu().double()
        assert torch.all((lp - logsm[idx]).abs() <= 1e-5), (nout, config, (lp - logsm[idx]).abs().max())
    assert torch.equal(action_index(act, nout), idx) and torch.equal(R.action_index(act, nout), idx)


# 3 ---------------------------------------------------------------------------------------------------------------------
def sampled_window(torch, env, actor, st):
    """`test_gpu_learner.rollout_window` that keeps what the acting kernel said: ``(out [T,E,N,nout], idx [T,E,N] or None, act [T,E,N,2])``,
    ``act`` a copy of each step's actions taken before the env stepped on them."""
    E = st.reward.shape[1]
    idx = torch.full((T, E, N), -1, dtype=torch.int32, device=DEV) if actor.out_kind == 1 else None
    outs, acts = [], []
    st.begin()
    for t in range(T):
        act, _, out = actor.sample_action(env.z, env=env, return_outputs=True, act_out=st.actions[t],
                                          idx_out=None if idx is None else idx[t])
        outs.append(out)
        acts.append(act.clone())
        env.step(st.actions[t], into=(st, t))
    return torch.stack(outs), idx, torch.stack(acts)


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("path", ["sa2c", ("PPOLearner", dict(epochs=1))], ids=["sa2c", "ppo-e1"])
@pytest.mark.parametrize("config", H.POLICY_CONFIGS)
def test_on_policy_identity_in_the_window_after_an_update(torch, config, path, kind):
    """Window 1 + ``train()``, then window 2 sampled with ``return_outputs=True``.  The log-probability the LEARNER's chain gives the stored
    actions on the stored ``z_pre`` (PPO: ``logp_old`` of window 2's ``train()``; SA2C: a `GradientRunner.logp` call before it) against
    what the ACTING kernel said when it sampled them:

      softmax    |exp(logp) - out[t, e, i, idx]| <= B, the configuration's bar on the acting kernel's output (1e-5; bf16 3e-2), every row
      Gaussian   logp against the float64 density of the stored action at the kernel's (mu, var), within the first-order propagation
                 B x sum_d (|a - mu| / var + (a - mu)^2 / (2 var^2) + 1 / (2 var)) + 1e-5 (1 + |logp|), on the rows whose float64
                 (mu, var) have var in [0.05, 0.95] and |mu| <= 0.98: at least 99 % of them

    It fails for a stale actor image (the kernel's probabilities are last window's), a wrong index and an action stored one slot away
    from its observation.  (The Gaussian comparison alone cannot see the last: any stored action has a density at the kernel's (mu, var).
    So the storage is also held, bit for bit, to a copy of each step's actions made before the env stepped on them.)  For PPO, window 2's ``V`` is the float64 forward of the critic as window 1's update left it."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    env, actor, critic, st, learner = build(torch, config, kind, path)
    E = S.envs_of(config)
    TG.rollout_window(env, actor, st)
    learner.train(st)
    torch.cuda.synchronize()
    assert every_env_ended_an_episode(st)
    out, idx, sampled = sampled_window(torch, env, actor, st)
    assert torch.equal(st.actions, sampled), "slot t of the storage does not hold the action sampled on slot t's observation"
    Wa, Wc = TP.weights_of(actor), TP.weights_of(critic)
    ppo = hasattr(learner, "logp_old")
    if not ppo:
        logp = GradientRunner(actor, T * E).logp(st.z_pre, st.actions, torch.empty(T, E, N, device=DEV)).clone()
    learner.train(st)
    torch.cuda.synchronize()
    if ppo:
        logp = learner.logp_old
    logp, out = logp.double().cpu(), out.double().cpu()
    B = S.out_bar(config)
    tag = f"{config} {'ppo' if ppo else 'sa2c'} {kind}:"
    assert torch.isfinite(logp).all()
    if kind == "softmax":
        idx = idx.cpu().long()
        assert int(idx.min()) >= 0 and int(idx.max()) < actor.nout
        p = out.gather(-1, idx[..., None])[..., 0]
        err = (torch.exp(logp) - p).abs()
        print(tag, f"worst |exp(logp) - p| = {float(err.max()):.3e} (bar {B:g}); indices seen: {idx.unique().numel()} of {actor.nout}")
        assert torch.all(err <= B), (tag, float(err.max()))
    else:
        x = st.z_pre.reshape(T * E, N, -1)
        inside = S.gaussian_region(S.forward64(Wa, x, kind)).reshape(T, E, N)
        share = float(inside.double().mean())
        ref, sens = S.gaussian_logp(st.actions.cpu(), out)
        excess = (logp - ref).abs() / (B * sens + 1e-5 * (1 + logp.abs()))
        print(tag, f"share of rows compared {share:.4f}; worst |logp - density| = {float(excess[inside].max()):.3f} bars")
        assert share >= 0.99
        assert torch.all(excess[inside] <= 1.0), (tag, float(excess[inside].max()))
    if ppo:
        V = learner.V.view(T * E, N, 1)
        miss = S.misses(V, S.forward64(Wc, st.z_pre.reshape(T * E, N, -1), "critic"), config)
        print(tag, f"window 2's V against the updated critic: worst {float(miss.max()):.3f} bars")
        assert torch.all(miss <= 1.0), (tag, miss)
