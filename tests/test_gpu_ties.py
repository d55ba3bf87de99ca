"""Neighbour-list ties with the self entry on every step geometry (fixtures and restatement: tests/ties_ref.py; the oracle is
pinned to the restatement by tests/test_ties_host.py).

A partner sorts at or ahead of the agent's own entry d_ii = min(-2 l_i, dhat_i) when it is exactly coincident (equal radii: an
exact tie, the lower index wins) or a larger agent over the smaller agent's centre (strictly ahead).  `NbrList<K, true>` of
csrc/drone_kernel.hpp -- the list form of kSym64, kBlock256, kBlockU256 and kBlock1024 at c = 2 with max Delta < min dhat --
handles both out of line: a wave-uniform general insertion, and the DEFER flag with blocks that start the walk over.  Which
start-over site a fixture reaches (read off the code; nothing instruments it):

  class          launch                pattern a / b (sparse)          pattern c (24-agent cluster)      d / e (nested)
  sym64          observe, step         after the per-lane walk         after the per-lane walk           --
  sym64          rollout               pair_phase (pairs listed once)  > 64 listed pairs: per-lane walk  --
  block, u256    observe, step         after walk() of the bucket      crowded: all-pairs fallback,      as a / b
                                       filter                          then the same block
  block, u256    rollout               the same, on the kept list      the same (list kept or rebuilt)   as a / b
                                       (CACHED_B)
  big            every launch          after walk() of the bucket      crowded: all-pairs fallback       as a / b
                                       filter, no kept list

Two coincident agents are also two partners of exactly equal distance in every third agent's row (lower index first).  The
cluster of pattern c is where these tests found the ascending-order list swapping such a pair: a closer partner of higher index
arrived later, and the shifted entry was compared with its equal instead of being moved along with the rest of the list.

In a workgroup-per-env class the verdict is per wave: pattern a puts the two agents in different waves for N > 64, so a wave
starts over while its siblings do not.  The four controls (packed, wave64, c = 5, Delta = dhat) order 64-bit (d, j) keys."""
import numpy as np
import pytest

from tests import helpers as H
from tests import ties_ref as R
from tests.test_gpu_f64 import TIGHT
from tests.test_gpu_parity import host, make_env
from tests.test_gpu_rollout_control_fuzz import geometry_class

pytestmark = pytest.mark.gpu

T = 12
OUTPUTS = ("reward", "true_reward", "z", "nbr_idx", "n_coll")
F64_CONFIGS = ["sym64-k2", "block-hetero", "big-hetero"]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def build_env(fx, n_envs=R.E, **kw):
    """The env of fixture `fx`, in the geometry class and the list form its table row names."""
    env = make_env(fx.N, fx.G, fx.k, fx.c, fx.delta, n_envs, **kw)
    if fx.hetero:
        env.drone_radius = fx.radius; env.d_safety = fx.d_hat; env.deltas = fx.delta
        for table, want in ((env._radius, fx.l), (env._d_hat, fx.d_hat), (env._delta, fx.orc.delta)):
            np.testing.assert_array_equal(host(table), want.astype(np.float32))
    p = env._params()
    assert geometry_class(env)[0] == fx.cls, (fx.name, geometry_class(env))
    asc = p.delta_max < p.d_hat_min and env.c == 2 and fx.cls in ("sym64", "block", "u256", "big")
    assert asc == fx.asc, (fx.name, p.delta_max, p.d_hat_min, env.c)
    return env


def outputs(env, done=False):
    got = {name: host(getattr(env, name)) for name in OUTPUTS + (("done",) if done else ())}
    got["z"] = got["z"].reshape(env.n_envs, env.n_agents, env.k_closest + 1, env.c)
    return got


def check(fx, got, ref, kept, what, tie_free=None):
    """Discrete outputs exactly, continuous ones at the suite's bars, on the `kept` envs -- tie envs included."""
    assert kept.any() and (kept & (fx.pat != "f")).any(), what
    for name in ("nbr_idx", "n_coll") + (("done",) if "done" in got else ()):
        bad = np.flatnonzero((np.asarray(got[name]) != np.asarray(ref[name])).reshape(kept.size, -1).any(1) & kept)
        assert bad.size == 0, f"{fx.name} {what}: {name} differs in envs {bad.tolist()} (patterns {fx.pat[bad].tolist()})"
    for name in ("reward", "true_reward"):
        H.assert_close(got[name][kept], ref[name][kept], f"{fx.name} {what} {name}", rtol=H.RTOL, atol=H.ATOL)
    tie_free = np.ones(ref["nbr_idx"].shape[:2], bool) if tie_free is None else tie_free
    m = H.z_compare_mask(ref["nbr_idx"], tie_free, fx.c)
    H.assert_close(np.where(m, got["z"], 0)[kept], np.where(m, ref["z"], 0)[kept], f"{fx.name} {what} z", rtol=H.RTOL,
                   atol=H.atol_coord(fx.G))


def oracle_step(fx, pos64, act):
    """Oracle.step from (pos64, 0, t = 0): the outputs with `done`, and the state it leaves."""
    pos, vel = pos64.copy(), np.zeros_like(pos64)
    ref = fx.orc.step(pos, vel, np.zeros(pos.shape[0], np.int32), act)
    ref["done"] = ref["done"].astype(bool)
    return ref, pos


def pool_actions(torch, fx, small, seed):
    """act [T, E, N, 2]: every member of a coincident (or nested) group gets its group's first row, so the members integrate
    identically and the pattern persists.  small: 0.02 U(-1, 1), the kept candidate list survives the rollout; otherwise the
    actions of test_rollout_with_pool_actions_equals_steps_across_resets, under which it is rebuilt."""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    act = torch.rand(T, R.E, fx.N, 2, device="cuda:0", generator=g) * 2 - 1
    if small:
        act *= 0.02
    else:
        act[::5] *= 3.0
        act[T // 3:T // 3 + 6, ::3] = 0.0
        act[T - 5] *= 30.0
    for e, groups in enumerate(fx.groups):
        for members in groups:
            act[:, e, members[1:]] = act[:, e, members[:1]]
    return act


def groups_coincide(fx, pos, envs):
    """The coincident groups (patterns a, b, c, e) of `envs` are still bitwise equal in pos [E, N, 2] (host, float32)."""
    seen = 0
    for e in envs:
        for members in fx.groups[e] if fx.pat[e] != "d" else []:
            assert (pos[e, members].view(np.uint32) == pos[e, members[0]].view(np.uint32)).all(), (fx.name, e, members)
            seen += 1
    return seen


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_single_launch_against_the_oracle(torch, name):
    """set_state (the observe path), then step(zeros) from the same state (the step path), against Oracle.observe / Oracle.step
    on the same float32 positions; and the control envs (f) bit-identical to a launch that holds only them."""
    fx = R.fixture(name)
    env = build_env(fx)
    zeros = torch.zeros(R.E, fx.N, 2, device="cuda:0")
    ref, pos1 = oracle_step(fx, fx.pos64, np.zeros_like(fx.pos64))
    assert np.array_equal(pos1, fx.pos64)
    for key in OUTPUTS:                                           # a step of zero actions observes the same state
        np.testing.assert_array_equal(ref[key], fx.ref[key])
    alone = fx.pat == "f"
    ctl = build_env(fx, int(alone.sum()))
    env.set_state(fx.pos); ctl.set_state(fx.pos[alone])
    torch.cuda.synchronize()
    check(fx, outputs(env), fx.ref, fx.kept, "observe", fx.row_tie_free)
    for key in OUTPUTS:
        assert torch.equal(getattr(env, key)[torch.as_tensor(alone)], getattr(ctl, key)), (name, "observe, control envs alone", key)
    env.step(zeros); ctl.step(zeros[:int(alone.sum())])
    torch.cuda.synchronize()
    assert np.array_equal(host(env.pos), fx.pos) and np.array_equal(host(env.t), np.ones(R.E, np.int32))
    got = outputs(env, done=True)
    got["done"] = got["done"].astype(bool)
    check(fx, got, ref, fx.kept, "step", fx.row_tie_free)
    for key in OUTPUTS + ("done", "pos"):
        assert torch.equal(getattr(env, key)[torch.as_tensor(alone)], getattr(ctl, key)), (name, "step, control envs alone", key)


@pytest.mark.parametrize("small", [True, False], ids=["small-actions", "large-actions"])
@pytest.mark.parametrize("auto", [False, True], ids=["plain", "auto-reset"])
@pytest.mark.parametrize("name", R.ASC_CONFIGS)
def test_rollout_equals_steps_while_the_tie_persists(torch, name, auto, small):
    """One launch of T steps against T launches of one step, bit for bit, with the members of every tie group driven by the same
    action row: the assertions of test_rollout_with_pool_actions_equals_steps_across_resets."""
    fx = R.fixture(name)
    kw = dict(auto_reset=True) if auto else {}
    a, b = build_env(fx, seed=321, **kw), build_env(fx, seed=321, **kw)
    rng = np.random.default_rng(fx.N + 7 * fx.k)
    t0 = rng.integers(150, 199, R.E).astype(np.int32) if auto else np.zeros(R.E, np.int32)
    if auto:
        t0[-1] = 199 - T // 2                                     # an episode ends in the middle of the rollout
    a.set_state(fx.pos, None, t0); b.set_state(fx.pos, None, t0)
    act = pool_actions(torch, fx, small, fx.N)
    out = a.rollout(act)
    for s in range(T):
        res = b.step(act[s])
        for key, ref in (("reward", res.rewards), ("true_reward", res.true_rewards), ("z", res.z_states),
                         ("nbr_idx", b.nbr_idx), ("n_coll", res.n_collisions), ("done", res.finished)):
            assert torch.equal(out[key][s], ref), (name, key, s)
    assert torch.equal(a.pos, b.pos) and torch.equal(a.t, b.t)
    done = host(out["done"]).astype(bool)
    assert done.any() == auto and (not auto or done[T // 2 - 1:T // 2 + 1, -1].any())
    # the subject of the test: the groups of the envs that were not re-sampled still coincide at the end
    alive = np.flatnonzero(~done.any(0))
    assert groups_coincide(fx, host(a.pos), alive) >= (3 if auto else 3 * R.E // 6)
    # ... and are still listed as such: some agent of every such tie env is listed among its own neighbours
    nb = host(out["nbr_idx"][T - 1])
    twice = (nb[:, :, 1:] == np.arange(fx.N)[None, :, None]).any((1, 2))
    assert twice[alive][fx.pat[alive] != "f"].all()


@pytest.mark.parametrize("name", R.ASC_CONFIGS)
def test_rollout_first_and_last_step_against_the_oracle(torch, name):
    """The anchor of the relative test above.  Step 0 of the pool carries zero actions, so out[...][0] is Oracle.step from the
    fixture's own state; out[...][T-1] was evaluated on the state the rollout leaves, which the oracle observes as float64."""
    fx = R.fixture(name)
    a = build_env(fx, seed=321)
    a.set_state(fx.pos)
    act = pool_actions(torch, fx, True, fx.N + 1)
    act[0] = 0.0
    out = a.rollout(act)
    torch.cuda.synchronize()
    shape = (R.E, fx.N, fx.k + 1, fx.c)
    pick = lambda s: {key: host(out[key][s]).reshape(shape) if key == "z" else host(out[key][s]) for key in OUTPUTS + ("done",)}
    ref, _ = oracle_step(fx, fx.pos64, np.zeros_like(fx.pos64))
    first = pick(0)
    first["done"] = first["done"].astype(bool)
    check(fx, first, ref, fx.kept, "rollout step 0")
    end = host(a.pos)
    assert groups_coincide(fx, end, range(R.E)) >= 3 * R.E // 6 and not np.array_equal(end, fx.pos)
    end64 = end.astype(np.float64)
    last = pick(T - 1)
    last["done"] = last["done"].astype(bool)
    ref_end = fx.orc.observe(end64, host(a.vel).astype(np.float64))
    ref_end["done"] = np.zeros(R.E, bool)                         # t = T < 199 and nobody near the goal ring
    kept = fx.kept_after(end64)
    for letter in sorted(set(fx.pat)):
        assert kept[fx.pat == letter].any(), (name, letter, "no env of the pattern is compared at the end of the rollout")
    check(fx, last, ref_end, kept, f"rollout step {T - 1}")


@pytest.mark.parametrize("name", F64_CONFIGS)
def test_float64_verification_kernel_on_ties(torch, name):
    """verify.F64Env, the suite's checker of float32 outputs, on the same fixtures: lists and counts exactly, rewards and z at
    its own bar."""
    from scalable_collision_avoidance_rl_amd.verify import F64Env
    fx = R.fixture(name)
    env = F64Env(fx.N, [fx.G, fx.G], fx.k, fx.delta, fx.c == 2, n_envs=R.E, device="cuda:0", drone_radius=fx.radius)
    np.testing.assert_array_equal(env.d_safety, fx.d_hat)
    np.testing.assert_array_equal(np.asarray(env.deltas, np.float64), fx.orc.delta)
    env.set_state(fx.pos64)
    torch.cuda.synchronize()
    kept = fx.kept
    np.testing.assert_array_equal(host(env.nbr_idx)[kept], fx.ref["nbr_idx"][kept])
    np.testing.assert_array_equal(host(env.n_coll)[kept], fx.ref["n_coll"][kept])
    H.assert_close(host(env.reward)[kept], fx.ref["reward"][kept], f"{name} f64 reward", **TIGHT)
    H.assert_close(host(env.true_reward)[kept], fx.ref["true_reward"][kept], f"{name} f64 true_reward", **TIGHT)
    H.assert_close(host(env.z).reshape(fx.ref["z"].shape)[kept], fx.ref["z"][kept], f"{name} f64 z", **TIGHT)
