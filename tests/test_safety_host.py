"""CPU checks of the per-episode safety tables: the float64 restatement of `dronesim_episode_safety`'s contract
(tests/safety_ref.py) against the reference's own clipped distance matrices (tests/golden/safety_n5.npz, written by
tests/golden/gen_safety_golden.py) and against a second, vectorised formulation; `episode_safety`'s argument checks that need no
device; the host side of `Evaluator.safety_summary`."""
import numpy as np
import pytest

from tests import safety_ref
from tests.helpers import load

EPISODES = ("p", "r", "s")


@pytest.mark.parametrize("a", EPISODES)
def test_safety_ref_reproduces_the_reference_distances(a):
    """The tables from z and Ni == the tables the generator derived from the reference's d_ij and state, within 1e-11."""
    fx = load("safety_n5.npz")
    z, nbr, done = safety_ref.golden_window(fx, a)
    ref = safety_ref.episode_safety(z, nbr, done, fx[f"{a}_radius"], fx[f"{a}_deltas"], float(fx["done_radius"]))
    assert ref["ep_len"][0] == int(fx[f"{a}_ep_len"]) and ref["ep_arrived"][0] == int(fx[f"{a}_ep_arrived"])
    assert np.array_equal(ref["arrive_step"][0], fx[f"{a}_arrive_step"])
    for name in ("min_clearance", "goal_dist_final"):
        err = np.abs(ref[name][0] - fx[f"{a}_{name}"]).max()
        print(f"episode {a} {name}: max error {err:.3e}")
        assert err <= 1e-11, (a, name, err)
    assert abs(ref["ep_min_clearance"][0] - fx[f"{a}_min_clearance"].min()) <= 1e-11
    assert abs(ref["ep_goal_dist_max"][0] - fx[f"{a}_goal_dist_final"].max()) <= 1e-11
    assert (int(fx[f"{a}_ep_collisions"]) == 0) == (ref["ep_min_clearance"][0] > 0)


def test_golden_holds_what_the_generator_promised():
    fx = load("safety_n5.npz")
    assert bool(fx["p_ep_arrived"]) and int(fx["p_ep_len"]) < 200 and int(fx["r_ep_len"]) == 200 and not bool(fx["r_ep_arrived"])
    assert fx["s_new_z"].shape[2] == 15 and fx["p_new_z"].shape[2] == 6
    assert any((fx[f"{a}_n_coll"] > 0).any() for a in EPISODES)
    assert any((fx[f"{a}_Ni"][:, :, 1] < 0).all(0).any() for a in EPISODES)
    assert ((fx["p_arrive_step"] > 0) & (fx["p_arrive_step"] < int(fx["p_ep_len"]))).any()


def vectorised(w, done_radius):
    """The same contract with array operations over the whole window (no loop over steps, envs or agents)."""
    z, nbr = w["z"].astype(np.float64), w["nbr"].astype(np.int64)
    T, E, N, k1 = nbr.shape
    c = z.shape[3] // k1
    done = w["done"] != 0
    L = np.where(done.any(0), done.argmax(0) + 1, 0)
    steps = np.arange(T)[:, None]
    if w["z_final"] is not None:
        last = (steps == L[None] - 1)[:, :, None, None]
        z, nbr = np.where(last, w["z_final"].astype(np.float64), z), np.where(last, w["nbr_final"].astype(np.int64), nbr)
    inside_ep = (steps < L[None])[:, :, None]                                   # [T,E,1]
    goal = np.hypot(z[..., 0], z[..., 1])
    j = nbr[..., 1]
    real = (j >= 0) & (j < N)
    gap = np.hypot(z[..., c], z[..., c + 1]) - w["radius"].astype(np.float64)[None, None] - w["radius"].astype(np.float64)[np.where(real, j, 0)]
    delta = np.broadcast_to(w["delta"].astype(np.float64), gap.shape)
    clr = np.where(real, np.minimum(gap, delta), delta)
    valid = L > 0
    fill = lambda x, v: np.where(valid.reshape((E,) + (1,) * (x.ndim - 1)), x, v)
    hit = inside_ep & (goal <= done_radius)
    final = np.take_along_axis(goal, np.broadcast_to(np.maximum(L - 1, 0)[None, :, None], (1, E, N)), 0)[0]
    out = dict(ep_len=L.astype(np.int32), min_clearance=fill(np.where(inside_ep, clr, np.inf).min(0), np.nan),
               goal_dist_final=fill(final, np.nan), arrive_step=np.where(hit.any(0), hit.argmax(0) + 1, -1).astype(np.int32))
    out["ep_min_clearance"] = out["min_clearance"].min(1)
    out["ep_goal_dist_max"] = out["goal_dist_final"].max(1)
    out["ep_arrived"] = (valid & ~(~(out["goal_dist_final"] <= done_radius)).any(1)).astype(np.uint8)
    return out


@pytest.mark.parametrize("shape", [(1, 1, 1, 2, 2), (7, 3, 4, 3, 2), (13, 11, 5, 3, 5), (9, 6, 8, 5, 2)])
@pytest.mark.parametrize("with_final", [False, True])
def test_safety_ref_matches_the_vectorised_formulation(shape, with_final):
    w = safety_ref.synthetic_window(*shape, seed=sum(shape), with_final=with_final)
    ref, vec = safety_ref.episode_safety(**w, done_radius=0.2), vectorised(w, 0.2)
    for name in safety_ref.TABLES:
        if ref[name].dtype.kind == "f":
            assert np.array_equal(np.isnan(ref[name]), np.isnan(vec[name])), name
            assert np.allclose(ref[name], vec[name], rtol=0, atol=1e-12, equal_nan=True), name
        else:
            assert np.array_equal(ref[name], vec[name]), name


def test_synthetic_windows_hold_every_case():
    w = safety_ref.synthetic_window(13, 10, 5, 3, 2, seed=2)
    per_env = w["done"].sum(0)
    assert (per_env == 0).any() and (per_env > 1).any() and w["done"][0].any() and ((per_env == 1) & (w["done"][-1] == 1)).any()
    j = w["nbr"][..., 1]
    assert (j == -1).any() and (j == 5).any() and (j > 5).any() and (j < -1).any() and ((j >= 0) & (j < 5)).any()
    assert np.isnan(w["z"]).sum() + np.isnan(w["z_final"]).sum() == 2
    assert len(set(w["radius"])) == 5 and len(set(w["delta"])) == 5
    ref = safety_ref.episode_safety(**w, done_radius=0.2)
    assert np.isnan(ref["min_clearance"][ref["ep_len"] > 0]).any() and np.isnan(ref["goal_dist_final"][ref["ep_len"] > 0]).any()
    assert np.isnan(ref["min_clearance"][ref["ep_len"] == 0]).all() and (ref["arrive_step"][ref["ep_len"] == 0] == -1).all()
    assert (ref["arrive_step"] > 0).any() and not ref["near"].any()
    assert set(ref["ep_arrived"][ref["ep_len"] > 0]) == {0, 1}


def test_episode_safety_checks_its_arguments_without_a_device():
    import torch
    from scalable_collision_avoidance_rl_amd.evaluate import SAFETY_TABLES, episode_safety
    assert set(SAFETY_TABLES) | {"ep_len"} == set(safety_ref.TABLES)
    T, E, N, k1, c = 4, 3, 5, 3, 2
    z, nbr, done = torch.zeros(T, E, N, k1 * c), torch.zeros(T, E, N, k1, dtype=torch.int32), torch.zeros(T, E, dtype=torch.uint8)
    r, d = torch.full((N,), 0.1), torch.ones(N)
    bad = [dict(z_final=z), dict(nbr_final=nbr), dict(done_radius=float("nan")), dict(z=z[..., :5]), dict(z=torch.zeros(T, E, N, 9)),
           dict(nbr=nbr[..., :1], z=z[..., :2]), dict(done=done[:3]), dict(radius=r[:4]), dict(delta=torch.ones(N, 1)),
           dict(z=z[:, :, :4]), dict(z_final=z[:3], nbr_final=nbr), dict(z=z.numpy())]
    for kw in bad:
        args = dict(z=z, nbr=nbr, done=done, radius=r, delta=d)
        args.update(kw)
        with pytest.raises(ValueError):
            episode_safety(**args)
    with pytest.raises(RuntimeError, match="device tensors"):               # well-formed host tensors: there is no CPU fallback
        episode_safety(z, nbr, done, r, d)


def test_summarize_safety_combines_ranks():
    import torch
    from scalable_collision_avoidance_rl_amd.evaluate import summarize_safety
    a = torch.tensor([2.0, 1.0, 1.0, 0.5, 0.1, 3.0, 4.0, 200.0], dtype=torch.float64)
    b = torch.tensor([6.0, 5.0, 2.0, 0.3, -0.2, 1.0, 26.0, 2800.0], dtype=torch.float64)
    s = summarize_safety(torch.stack([a, b]))
    assert s["episodes"] == 8 and s["world_size"] == 2 and s["arrived_share"] == 0.75 and s["success_share"] == 0.375
    assert s["min_clearance"] == -0.2 and abs(s["mean_min_clearance"] - 0.1) < 1e-15 and s["mean_goal_dist_max"] == 0.5
    assert s["mean_arrive_step"] == 100.0
    idle = torch.tensor([0.0, 0, 0, 0, float("inf"), 0, 0, 0], dtype=torch.float64)      # a rank without an episode
    assert summarize_safety(torch.stack([a, idle]))["min_clearance"] == 0.1
    none = summarize_safety(idle[None])
    assert none["episodes"] == 0 and none["min_clearance"] is None and none["mean_arrive_step"] is None
