"""Per-episode safety tables on the device: `dronesim_episode_safety` (csrc/evaluate.hip), `evaluate.episode_safety`,
`RolloutStorage.safety` and `Evaluator(safety=True)` against the float64 restatement tests/safety_ref.py, the reference's own
distance matrices (tests/golden/safety_n5.npz), `dronesim_episode_ends` and `episode_eval` on real rollouts."""
import ctypes as C

import numpy as np
import pytest

from tests import safety_ref
from tests import helpers as H

pytestmark = pytest.mark.gpu
ATOL = 1e-5                  # the project's standing agreement with the CPU reference (tests/helpers.py)
CAP = 0.01                   # the share of entries that may be left out because a decision sits on its threshold
FLOATS = ("min_clearance", "goal_dist_final", "ep_min_clearance", "ep_goal_dist_max")

# (T, E, N, k1, c, z_final?, byte offset of z, byte offset of z_final) -- the smallest windows that reach every path:
#   load width   16 bytes: c = 2, k1 even, both bases 16-byte aligned; 8 bytes: c = 2 and k1 odd, or a base at 8 (mod 16);
#                4 bytes: a base at 4 (mod 8), and every c = 5 window
#   flag fetch   cooperative when a wave's 64 columns span at most 8 envs (N = 8: a wave straddles 8 envs; N = 64), own loads
#                otherwise (N = 1, 4, 5)
#   stages       T = 1, 7 (a remainder), 8 (exactly one stage of kStageT), 13 (one stage and a remainder)
#   blocks       E N = 350, 560: more than one workgroup with a ragged last one
WINDOWS = [(1, 1, 1, 2, 2, True, 0, 0), (7, 3, 4, 2, 2, True, 0, 0), (8, 70, 5, 2, 2, False, 0, 0), (13, 70, 8, 2, 2, True, 0, 0),
           (13, 3, 8, 2, 2, True, 8, 0), (7, 70, 8, 2, 2, True, 0, 8), (8, 3, 5, 2, 2, False, 4, 0), (13, 70, 4, 2, 2, True, 8, 4),
           (13, 70, 5, 5, 2, True, 0, 0), (8, 3, 8, 5, 2, True, 4, 4), (7, 1, 4, 5, 2, False, 8, 0),
           (13, 70, 5, 5, 5, True, 0, 0), (8, 3, 8, 2, 5, True, 4, 8), (7, 70, 1, 2, 5, False, 8, 0), (1, 3, 4, 5, 5, True, 0, 4),
           (13, 3, 64, 2, 2, True, 0, 0)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def host(t):
    return t.detach().cpu().numpy()


def at_offset(torch, a, nbytes):
    """`a` on the device, contiguous, its base `nbytes` past a 16-byte boundary."""
    t = torch.as_tensor(a)
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0 and nbytes % 4 == 0
    view = buf[nbytes // 4: nbytes // 4 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == nbytes and view.is_contiguous()
    return view


def check_tables(got, ref, what, near=None):
    """ep_len exact; the float tables within 1e-5 with NaN where the restatement has NaN; arrive_step / ep_arrived exact outside
    the entries `near` marks (a goal distance within 4 float32 ulps of the disk's radius), of which there may be at most 1 %."""
    assert np.array_equal(host(got["ep_len"]), ref["ep_len"]), what
    for name in FLOATS:
        g, r = host(got[name]).astype(np.float64), ref[name]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, name)
        err = np.abs(g - r)[~np.isnan(r)].max(initial=0.0)
        print(f"{what} {name}: max error {err:.3e}")
        assert err <= ATOL, (what, name, err)
    near = np.zeros(ref["arrive_step"].shape, bool) if near is None else near
    assert near.mean() <= CAP and near.any(1).mean() <= CAP, (what, near.mean())
    assert np.array_equal(host(got["arrive_step"])[~near], ref["arrive_step"][~near]), what
    assert np.array_equal(host(got["ep_arrived"])[~near.any(1)], ref["ep_arrived"][~near.any(1)]), what


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("case", WINDOWS, ids=lambda s: "x".join(map(str, s)))
def test_episode_safety_kernel_matches_safety_ref(torch, case):
    from scalable_collision_avoidance_rl_amd.evaluate import episode_safety
    T, E, N, k1, c, with_final, off_z, off_f = case
    w = safety_ref.synthetic_window(T, E, N, k1, c, seed=WINDOWS.index(case), with_final=with_final)
    ref = safety_ref.episode_safety(**w, done_radius=0.2)
    d = {k: None if v is None else torch.as_tensor(v, device="cuda:0") for k, v in w.items()}
    d["z"] = at_offset(torch, w["z"], off_z)
    if with_final:
        d["z_final"] = at_offset(torch, w["z_final"], off_f)
    out = episode_safety(**d, done_radius=0.2)
    again = episode_safety(**d, done_radius=0.2)
    for name in out:                                                        # bit-identical run to run
        assert torch.equal(out[name].view(torch.uint8), again[name].view(torch.uint8)), name
    check_tables(out, ref, f"window {case}", ref["near"])
    none = ref["ep_len"] == 0                                               # no episode: NaN, -1, 0
    assert np.isnan(host(out["min_clearance"])[none]).all() and (host(out["arrive_step"])[none] == -1).all()
    assert not host(out["ep_arrived"])[none].any() and np.isnan(host(out["ep_min_clearance"])[none]).all()
    # outputs left out are not computed; ep_len alone works
    few = dict(ep_len=torch.full_like(out["ep_len"], -7), arrive_step=torch.full_like(out["arrive_step"], -7))
    episode_safety(**d, done_radius=0.2, out=few)
    assert torch.equal(few["ep_len"], out["ep_len"]) and torch.equal(few["arrive_step"], out["arrive_step"])


def test_ghost_ids_never_count(torch):
    """-1, N, a large id and a negative one in slot 1 all give Delta, whatever row 1 holds."""
    from scalable_collision_avoidance_rl_amd.evaluate import episode_safety
    T, E, N, k1, c = 7, 3, 5, 3, 2
    w = safety_ref.synthetic_window(T, E, N, k1, c, seed=1, with_final=False)
    w["done"][:] = 0
    w["done"][T - 1] = 1
    w["z"] = np.nan_to_num(w["z"])
    for e, j in enumerate((-1, N, 2 ** 31 - 1)):
        w["nbr"][:, e, :, 1] = j
    w["nbr"][0, 2, :, 1] = -(2 ** 31)
    out = episode_safety(**{k: None if v is None else torch.as_tensor(v, device="cuda:0") for k, v in w.items()})
    assert np.array_equal(host(out["min_clearance"]), np.broadcast_to(w["delta"], (E, N)))
    assert np.array_equal(host(out["ep_min_clearance"]), np.full(E, w["delta"].min()))


def test_episode_safety_rejects_bad_arguments(torch):
    from scalable_collision_avoidance_rl_amd import _native
    from scalable_collision_avoidance_rl_amd.evaluate import episode_safety
    T, E, N, k1, c = 4, 3, 5, 3, 2
    w = safety_ref.synthetic_window(T, E, N, k1, c, seed=0)
    d = {k: torch.as_tensor(v, device="cuda:0") for k, v in w.items()}
    lib = _native.lib()
    out = episode_safety(**d)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        a = dict(z=d["z"].data_ptr(), nbr=d["nbr"].data_ptr(), z_final=d["z_final"].data_ptr(), nbr_final=d["nbr_final"].data_ptr(),
                 done=d["done"].data_ptr(), radius=d["radius"].data_ptr(), delta=d["delta"].data_ptr(), done_radius=0.2, T=T, E=E, N=N,
                 k1=k1, c=c, ep_len=out["ep_len"].data_ptr(), min_clearance=out["min_clearance"].data_ptr(),
                 goal_dist_final=out["goal_dist_final"].data_ptr(), arrive_step=out["arrive_step"].data_ptr(),
                 ep_min_clearance=out["ep_min_clearance"].data_ptr(), ep_goal_dist_max=out["ep_goal_dist_max"].data_ptr(),
                 ep_arrived=out["ep_arrived"].data_ptr())
        a.update(kw)
        return lib.dronesim_episode_safety(*a.values(), stream)

    assert call() == _native.OK
    for kw in (dict(z=None), dict(nbr=None), dict(done=None), dict(radius=None), dict(delta=None), dict(ep_len=None), dict(k1=1),
               dict(c=3), dict(c=0), dict(N=0), dict(N=1025), dict(T=-1), dict(E=-1), dict(done_radius=float("nan")),
               dict(z_final=None), dict(nbr_final=None), dict(min_clearance=None), dict(goal_dist_final=None)):
        assert call(**kw) == _native.EINVAL, kw
    assert b"dronesim_episode_safety" in lib.dronesim_last_error()
    assert call(z_final=None, nbr_final=None) == _native.OK
    assert call(goal_dist_final=None, ep_goal_dist_max=None, ep_arrived=None) == _native.OK
    assert call(E=0) == _native.OK
    # T = 0: the L = 0 values are written
    for t in out.values():
        t.fill_(3)
    assert call(T=0) == _native.OK
    assert not host(out["ep_len"]).any() and np.isnan(host(out["min_clearance"])).all() and np.isnan(host(out["ep_goal_dist_max"])).all()
    assert (host(out["arrive_step"]) == -1).all() and not host(out["ep_arrived"]).any()
    with pytest.raises(ValueError):
        episode_safety(**d, out=dict(ep_len=torch.zeros(E + 1, dtype=torch.int32, device="cuda:0")))


# ---------------------------------------------------------------------------------------------- 2. the reference's episodes
@pytest.mark.parametrize("a", ["p", "r", "s"])
def test_kernel_reproduces_the_reference_distances(torch, a):
    """The kernel on the golden's float32 z == the tables derived from the reference's d_ij and state, within 1e-5; the arrival
    steps exactly (the generator keeps every goal distance 1e-5 away from the disk's radius)."""
    from scalable_collision_avoidance_rl_amd.evaluate import episode_safety
    fx = H.load("safety_n5.npz")
    z, nbr, done = safety_ref.golden_window(fx, a, dtype=np.float32)
    dev = lambda x, dt: torch.as_tensor(np.asarray(x), dtype=dt, device="cuda:0")
    out = episode_safety(dev(z, torch.float32), dev(nbr, torch.int32), dev(done, torch.uint8), dev(fx[f"{a}_radius"], torch.float32),
                         dev(fx[f"{a}_deltas"], torch.float32), done_radius=float(fx["done_radius"]))
    assert int(out["ep_len"][0]) == int(fx[f"{a}_ep_len"]) and int(out["ep_arrived"][0]) == int(fx[f"{a}_ep_arrived"])
    assert np.array_equal(host(out["arrive_step"])[0], fx[f"{a}_arrive_step"])
    for name, want in (("min_clearance", fx[f"{a}_min_clearance"]), ("goal_dist_final", fx[f"{a}_goal_dist_final"]),
                       ("ep_min_clearance", fx[f"{a}_min_clearance"].min()), ("ep_goal_dist_max", fx[f"{a}_goal_dist_final"].max())):
        err = np.abs(host(out[name])[0].astype(np.float64) - want).max()
        print(f"episode {a} {name}: max error {err:.3e}")
        assert err <= ATOL, (a, name, err)


# ---------------------------------------------------------------------------------------------- 3. real rollouts
def make_env(N, E, seed, **kw):
    from scalable_collision_avoidance_rl_amd import drones
    return drones(N, 0, [5, 5], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True, device="cuda:0",
                  seed=seed, **kw)


@pytest.mark.parametrize("N", [5, 8])
@pytest.mark.parametrize("actions", ["proportional", "random"])
@pytest.mark.parametrize("auto_reset", [False, True])
def test_safety_of_real_rollouts(torch, auto_reset, actions, N):
    from scalable_collision_avoidance_rl_amd.drone_env import DONE_RADIUS
    from scalable_collision_avoidance_rl_amd.evaluate import episode_eval
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage, episode_ends
    E, T = 64, 200

    def window(auto_reset):
        env = make_env(N, E, 11, auto_reset=auto_reset)
        st = RolloutStorage(env, T, actions=True)
        if actions == "proportional":
            env.rollout_control("proportional", T, record_actions=True, into=st)
        else:
            g = torch.Generator(device="cuda:0").manual_seed(N)
            st.actions.copy_(torch.rand(st.actions.shape, generator=g, device="cuda:0") * 2 - 1)
            st.begin()
            for t in range(T):
                env.step(st.actions[t], into=(st, t))
        return env, st

    env, st = window(auto_reset)
    out = st.safety()
    twin = window(not auto_reset)[1].safety()                               # an env's first episode does not depend on auto_reset:
    for name in out:                                                        # z_final[t] under it == z[t] without it, bit for bit
        assert torch.equal(out[name], twin[name]), name
    assert (st.z_final is not None) == auto_reset
    ev = episode_eval(st.reward, st.true_reward, st.n_coll, st.done, None, 0.99, want_G=False)
    L = host(out["ep_len"]).astype(np.int64)
    assert np.array_equal(L, host(ev["ep_len"])) and (L > 0).all()
    # ep_arrived == the kind of each env's first end, bit for bit (without auto_reset z[t] IS the terminal observation)
    ends = host(episode_ends(st.done, st.z_final if auto_reset else st.z, DONE_RADIUS, 1)[0])
    first = ends[L - 1, np.arange(E)]
    assert np.array_equal(host(out["ep_arrived"]), (first == 1).astype(np.uint8)) and (first > 0).all()
    assert host(out["ep_arrived"]).any() == (actions == "proportional")       # random walks end at the time limit
    # a collision is a negative clearance
    clr = host(out["ep_min_clearance"]).astype(np.float64)
    sure = np.abs(clr) > ATOL
    assert (~sure).mean() <= CAP
    assert np.array_equal(host(ev["ep_collisions"])[sure] == 0, clr[sure] > 0)
    assert (host(out["min_clearance"]) <= host(env._delta)[None]).all()
    # and the tables of the first 16 envs against the restatement on the stored observations
    cut = lambda t: None if t is None else host(t)[:, :16]
    ref = safety_ref.episode_safety(cut(st.z), cut(st.nbr_idx), cut(st.done), host(env._radius), host(env._delta), DONE_RADIUS,
                                    cut(st.z_final), cut(st.nbr_final))
    check_tables({k: v[:16] for k, v in out.items()}, ref, f"rollout {actions} N={N} auto_reset={auto_reset}", ref["near"])
    print(f"{actions} N={N} auto_reset={auto_reset}: arrived {int(out['ep_arrived'].sum())}/{E}, episodes with a collision "
          f"{int((host(ev['ep_collisions']) > 0).sum())}, smallest clearance {clr.min():.4f}")


# ---------------------------------------------------------------------------------------------- 4. Evaluator(safety=True)
def networks(torch, N, d_in):
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    g = torch.Generator().manual_seed(0)
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * 0.2
    return BatchedMLP(r(N, d_in, 300), r(N, 300), r(N, 300, 300), r(N, 300), r(N, 300, 16), r(N, 16), 1, 1, device="cuda:0", seed=5)


def test_evaluator_safety_tables(torch):
    """The tables of a round == episode_safety on its storage; two evaluators with the same seeds agree bit for bit; the
    default Evaluator returns exactly the keys it returned before and has no safety summary."""
    from scalable_collision_avoidance_rl_amd.evaluate import SAFETY_TABLES, Evaluator, episode_safety
    N, E = 5, 16
    evs = [Evaluator(make_env(N, E, 29, auto_reset=True), "proportional", safety=True) for _ in range(2)]
    tabs = [ev.run(2) for ev in evs]
    plain = Evaluator(make_env(N, E, 29, auto_reset=True), "proportional")
    base = plain.run(2)
    assert set(base) == {"ep_len", "ep_collisions", "ep_return", "ep_true_return", "agent_return", "agent_true_return", "collision_hist"}
    assert set(tabs[0]) == set(base) | set(SAFETY_TABLES)
    for name in base:
        assert torch.equal(base[name], tabs[0][name]), name
    for name in tabs[0]:                                                    # (bit patterns: the tables hold no NaN here anyway)
        assert torch.equal(tabs[0][name], tabs[1][name]), name
    st = evs[0].storage                                                     # holds the second round
    direct = episode_safety(st.z, st.nbr_idx, st.done, st.env._radius, st.env._delta, st.z_final, st.nbr_final)
    for name in SAFETY_TABLES:
        assert tabs[0][name].shape[:2] == (2, E) and torch.equal(tabs[0][name][1], direct[name]), name
    assert not torch.equal(tabs[0]["min_clearance"][0], tabs[0]["min_clearance"][1])
    ptrs = {k: v.data_ptr() for k, v in tabs[0].items()}                    # allocated once
    assert {k: v.data_ptr() for k, v in evs[0].run(2).items()} == ptrs
    with pytest.raises(RuntimeError):
        plain.safety_summary()
    s, t = evs[1].safety_summary(), tabs[1]
    arrived = host(t["ep_arrived"]) != 0
    assert s["episodes"] == 2 * E and s["world_size"] == 1 and s["arrived_share"] == arrived.mean()
    assert s["success_share"] == (arrived & (host(t["ep_collisions"]) == 0)).mean()
    assert s["min_clearance"] == float(host(t["ep_min_clearance"]).min())
    assert abs(s["mean_min_clearance"] - host(t["ep_min_clearance"]).astype(np.float64).mean()) < 1e-12
    assert abs(s["mean_goal_dist_max"] - host(t["ep_goal_dist_max"]).astype(np.float64).mean()) < 1e-12
    steps = host(t["arrive_step"])
    assert abs(s["mean_arrive_step"] - steps[steps > 0].mean()) < 1e-9
    assert set(evs[1].summary()) == set(plain.summary())


def test_evaluator_safety_round_replays_from_a_graph(torch):
    """One round with safety=True captured in a graph: its replay == the eager round of a twin at the same episode counters."""
    from scalable_collision_avoidance_rl_amd.evaluate import SAFETY_TABLES, Evaluator
    N, E = 5, 6
    envs = [make_env(N, E, 9, auto_reset=True) for _ in range(2)]
    actor = networks(torch, N, envs[0].local_state_space)
    eager, graphed = (Evaluator(e, actor, safety=True) for e in envs)
    eager.run(1); graphed.run(1)                                            # warm-up round: buffers exist, counters agree
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tab_g = graphed.run(1)
    tab_e = {k: v.clone() for k, v in eager.run(1).items()}
    graph.replay()
    torch.cuda.synchronize()
    assert set(SAFETY_TABLES) <= set(tab_e)
    for name in tab_e:
        assert torch.equal(tab_e[name], tab_g[name]), name
    assert torch.equal(eager.storage.zbuf, graphed.storage.zbuf)
