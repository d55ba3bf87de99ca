"""Action shield on the device: `dronesim_action_shield` / `dronesim_shield_totals` (csrc/shield.hip), `ActionShield`,
`drones.step(execute=)` and `Evaluator(shield=)` against the float64 brute-force restatement tests/shield_ref.py.

Per record the kernel's answer must be FEASIBLE for the restatement's constraints (a.u* - b <= tol) and OPTIMAL (|u* - u| <=
|u_ref - u| + tol) with the derived bar tol = 16 eps32 (max(|u|inf, u_max) + rate (D + 2 l_max + margin) / dt)
(`shield_ref.tolerance`); pass-through is bit for bit; the intervened flag agrees on every record whose smallest float64 slack
exceeds tol (the others, at most 2 % of a case, are left out of the flag comparison only)."""
import types

import numpy as np
import pytest

from tests import shield_ref as S

pytestmark = pytest.mark.gpu
BAND_CAP = 0.02


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def refs():
    return {case: S.case_reference(*case) for case in S.CASES}


def host(t):
    return t.detach().cpu().numpy()


def dev(torch, a, offset=0):
    """`a` on the device, contiguous, its base `offset` bytes past a 16-byte boundary."""
    t = torch.as_tensor(a)
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0 and offset % 4 == 0
    view = buf[offset // 4: offset // 4 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    return view


def stand_in_env(torch, E, N, k, c, radius):
    """What `ActionShield` reads of an env, for record shapes no `drones` env has (N = 1)."""
    return types.SimpleNamespace(batched=True, n_envs=E, n_agents=N, k_closest=k, c=c, device=torch.device("cuda", 0), z=None,
                                 nbr_idx=None, _radius=torch.as_tensor(radius, device="cuda:0"))


def make_env(N, E, seed, k=2, c2=True, grid=(5, 5), **kw):
    from scalable_collision_avoidance_rl_amd import drones
    kw.setdefault("deltas", np.ones(N))
    return drones(N, 0, list(grid), "O", k_closest=k, simplify_zstate=c2, n_envs=E, batched=True, device="cuda:0",
                  seed=seed, **kw)


def check_against_ref(what, out, iv, corr, u, z, nbr, radius, c, rate=S.RATE, margin=S.MARGIN, u_max=S.U_MAX, ref=None):
    """The per-record bars of the module docstring; `out`, `iv`, `corr`: the kernel's arrays, `u`, `z`, `nbr`: what it read."""
    R, k1 = nbr.shape[0] * nbr.shape[1], nbr.shape[2]
    u2, z2, nbr2 = u.reshape(R, 2), z.reshape(R, k1 * c), nbr.reshape(R, k1)
    o, iv, corr = out.reshape(R, 2), iv.reshape(R).astype(bool), corr.reshape(R)
    if ref is None:
        ustar, riv, rcorr, slack = S.shield(u2, z2, nbr2, radius, rate, margin, u_max, S.DT, c)
        A, B, _ = S.constraints(z2, nbr2, radius, rate, margin, u_max, S.DT, c)
        tol = S.tolerance(u2, z2, k1, c, radius, rate, margin, u_max, S.DT)
    else:
        ustar, riv, rcorr, slack, A, B, tol = (ref[n] for n in ("ustar", "intervened", "correction", "min_slack", "A", "B", "tol"))
    fin = np.isfinite(u2).all(1)
    o64, u64 = o.astype(np.float64), u2.astype(np.float64)
    feas = ((A[fin] * o64[fin][:, None, :]).sum(2) - B[fin]).max(initial=-np.inf)
    with np.errstate(invalid="ignore"):
        d_got, d_ref = np.linalg.norm(o64 - u64, axis=1), np.linalg.norm(ustar - u64, axis=1)
    opt = (d_got - d_ref)[fin].max(initial=-np.inf)
    band = slack <= tol
    print(f"{what}: tol {tol:.3e}; feasibility residual {feas:.3e} ({feas / tol:.3f} tol); optimality excess {opt:.3e} "
          f"({opt / tol:.3f} tol); intervened {iv.mean():.3f}; flag band {band.mean():.4f}")
    assert feas <= tol, (what, feas, tol)
    assert opt <= tol, (what, opt, tol)
    assert band.mean() <= BAND_CAP, (what, band.mean())
    assert np.array_equal(iv[~band], riv[~band]), what
    # pass-through: u's own bits, correction 0; a non-finite u: copied through, flag 0, correction NaN
    assert np.array_equal(o[~iv].view(np.uint32), u2[~iv].view(np.uint32)), what
    assert (corr[~iv & fin] == 0).all() and np.isnan(corr[~fin]).all() and not iv[~fin].any(), what
    assert np.abs(corr[iv].astype(np.float64) - d_got[iv]).max(initial=0.0) <= tol, what
    return tol


# ---------------------------------------------------------------------------------------------- 1. the kernel, synthetic records
@pytest.mark.parametrize("case", S.CASES, ids=lambda c: "N%dk%dc%d" % c)
def test_kernel_matches_the_restatement_on_synthetic_records(torch, refs, case):
    from scalable_collision_avoidance_rl_amd import ActionShield
    N, k, c = case
    r = refs[case]
    sh = ActionShield(stand_in_env(torch, S.E_CASE, N, k, c, r["radius"]), S.RATE, S.MARGIN, S.U_MAX)
    u, z, nbr = dev(torch, r["u"]), dev(torch, r["z"]), dev(torch, r["nbr"])
    out = sh(u, z=z, nbr=nbr)
    check_against_ref(f"synthetic {case}", host(out), host(sh.intervened), host(sh.correction), r["u"], r["z"], r["nbr"], r["radius"], c,
                      ref=r)


@pytest.mark.parametrize("offset", [4, 8])
def test_kernel_reads_z_at_a_base_that_breaks_the_alignment(torch, refs, offset):
    """(2, 1, 2): 16-byte records; a base at 8 (mod 16) takes the 8-byte loads, at 4 (mod 8) the dword loads -- same bits."""
    from scalable_collision_avoidance_rl_amd import ActionShield
    N, k, c = case = S.CASES[0]
    r = refs[case]
    sh = ActionShield(stand_in_env(torch, S.E_CASE, N, k, c, r["radius"]), S.RATE, S.MARGIN, S.U_MAX)
    u, nbr = dev(torch, r["u"]), dev(torch, r["nbr"])
    aligned = sh(u, z=dev(torch, r["z"]), nbr=nbr)
    iv = sh.intervened.clone()
    shifted = sh(u, z=dev(torch, r["z"], offset), nbr=nbr)
    assert torch.equal(aligned.view(torch.int32), shifted.view(torch.int32)) and torch.equal(iv, sh.intervened)
    check_against_ref(f"z at +{offset}", host(shifted), host(sh.intervened), host(sh.correction), r["u"], r["z"], r["nbr"], r["radius"],
                      c, ref=r)
    # actions at a base that breaks their 8-byte alignment: the same bits through dword accesses
    odd = sh(dev(torch, r["u"], 4), z=dev(torch, r["z"]), nbr=nbr)
    assert torch.equal(aligned.view(torch.int32), odd.view(torch.int32))


def test_without_a_box_only_the_neighbours_bind(torch, refs):
    from scalable_collision_avoidance_rl_amd import ActionShield
    N, k, c = case = (5, 2, 2)
    r = refs[case]
    sh = ActionShield(stand_in_env(torch, S.E_CASE, N, k, c, r["radius"]), S.RATE, S.MARGIN, None)
    out = sh(dev(torch, r["u"]), z=dev(torch, r["z"]), nbr=dev(torch, r["nbr"]))
    check_against_ref("no box", host(out), host(sh.intervened), host(sh.correction), r["u"], r["z"], r["nbr"], r["radius"], c,
                      u_max=np.inf)


# ---------------------------------------------------------------------------------------------- 2. real observations
@pytest.mark.parametrize("N,E", [(5, 37), (64, 24)])
def test_kernel_on_real_observations_env_and_storage_slots(torch, N, E):
    from scalable_collision_avoidance_rl_amd import ActionShield
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    # (N = 64 on a 12 x 12 grid: the goal ring leaves Delta = d_hat = 0.32, and the lattice is dense enough for listed neighbours)
    env = make_env(N, E, 11, grid=(5, 5) if N == 5 else (12, 12), deltas=None if N == 64 else np.ones(N))
    st = RolloutStorage(env, 4)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    draw = lambda: (torch.rand(E, N, 2, device="cuda:0", generator=g) * 3 - 1.5)
    for _ in range(6):                                                             # some random steps off the lattice
        env.step(draw())
    sh = ActionShield(env, S.RATE, S.MARGIN, S.U_MAX)
    radius = host(env._radius)
    u = draw()
    out = sh(u)                                                                    # the env's own z / nbr_idx
    listed = S.constraints(host(env.z).reshape(E * N, -1), host(env.nbr_idx).reshape(E * N, -1), radius, S.RATE, S.MARGIN, S.U_MAX,
                           S.DT, 2)[2][:, S.M_BOX:]
    print(f"N={N}: records with a listed neighbour {listed.any(1).mean():.3f}")
    assert listed.any(1).mean() >= 0.1
    check_against_ref(f"env N={N}", host(out), host(sh.intervened), host(sh.correction), host(u), host(env.z), host(env.nbr_idx),
                      radius, 2)
    st.begin()
    for t in range(4):
        env.step(draw(), into=(st, t))
    for slot in (1, 4):                                                            # ring slots: bases inside one big allocation
        u = draw()
        out = sh(u, z=st.zbuf[slot], nbr=st.nbrbuf[slot])
        check_against_ref(f"storage slot {slot} N={N}", host(out), host(sh.intervened), host(sh.correction), host(u),
                          host(st.zbuf[slot]), host(st.nbrbuf[slot]), radius, 2)


def test_ghosts_self_zero_distance_nan_rows_and_nan_actions(torch):
    """Hand-placed: ghost ids (-1, N, the int32 extremes), the self id, d = 0 and a NaN neighbour row are skipped -- whatever the
    row holds, radius is never indexed with the id --, a NaN / inf action is copied through with correction NaN and counted."""
    from scalable_collision_avoidance_rl_amd import ActionShield
    N, E = 5, 8
    env = make_env(N, E, 5)
    sh = ActionShield(env, S.RATE, S.MARGIN, S.U_MAX, stats=True)
    z, nbr = env.z.clone().view(E, N, 3, 2), env.nbr_idx.clone()
    z[:, :, 1] = torch.tensor([0.26, 0.0])                                         # every agent: a neighbour 0.26 to the right, g = 0.01
    z[:, :, 2] = torch.tensor([0.0, 0.3])                                          # and one 0.3 above, g = 0.05
    ids = torch.arange(N, device="cuda:0", dtype=torch.int32)
    nbr[:, :, 1] = (ids + 1) % N
    nbr[:, :, 2] = (ids + 2) % N
    u = torch.full((E, N, 2), 0.9, device="cuda:0")
    for e, j in enumerate((-1, N, 2 ** 31 - 1, -2 ** 31)):                         # envs 0..3: slot 1 a ghost
        nbr[e, :, 1] = j
    nbr[4, :, 1] = ids                                                             # env 4: slot 1 names the agent itself
    z[5, :, 1] = 0.0                                                               # env 5: d = 0
    z[6, :, 1, 0] = float("nan")                                                   # env 6: a NaN row
    u[7, 0, 0], u[7, 1, 1], u[7, 2, 0] = float("nan"), float("inf"), float("-inf")  # env 7: non-finite actions
    z = z.view(E, N, 6)
    out = sh(u, z=z, nbr=nbr)
    check_against_ref("hand-placed", host(out), host(sh.intervened), host(sh.correction), host(u), host(z), host(nbr), host(env._radius), 2)
    o = host(out)
    # slot 1 skipped: only slot 2 binds, u* = (0.9, b2) with b2 = rate 0.05 / dt = 0.25
    assert np.allclose(o[:7, :, 0], 0.9) and np.allclose(o[:7], [0.9, 0.25], atol=1e-5)
    assert np.allclose(o[7, 3:], [0.05, 0.25], atol=1e-5)                          # both bind: b1 = rate 0.01 / dt = 0.05
    assert np.array_equal(o[7, :3].view(np.uint32), host(u)[7, :3].view(np.uint32))
    t = sh.totals()
    assert host(t["nonfinite"]).tolist() == [1, 1, 1, 0, 0] and host(t["interventions"]).tolist() == [7, 7, 7, 8, 8]


# ---------------------------------------------------------------------------------------------- 3. aliasing, determinism, totals
def test_aliasing_determinism_and_totals(torch, refs):
    from scalable_collision_avoidance_rl_amd import ActionShield
    N, k, c = case = (9, 8, 2)
    r = refs[case]
    u_np = r["u"].copy()
    u_np[3, 2, 0] = np.nan                                                         # one non-finite action
    z, nbr = dev(torch, r["z"]), dev(torch, r["nbr"])
    runs = []
    for _ in range(2):
        sh = ActionShield(stand_in_env(torch, S.E_CASE, N, k, c, r["radius"]), S.RATE, S.MARGIN, S.U_MAX, stats=True)
        u = dev(torch, u_np)
        out = sh(u, z=z, nbr=nbr)
        iv1, c1 = host(sh.intervened).copy(), host(sh.correction).copy()
        inplace = u.clone()
        assert sh(inplace, z=z, nbr=nbr, out=inplace) is inplace                   # out aliases actions
        assert torch.equal(inplace.view(torch.int32), out.view(torch.int32))
        iv2, c2 = host(sh.intervened).copy(), host(sh.correction).copy()
        assert np.array_equal(iv1, iv2) and np.array_equal(c1.view(np.uint32), c2.view(np.uint32))
        runs.append((out, sh.totals(), sh))
        # the totals of the two calls against float64 sums of the kernel's own planes
        t = {n: host(v) for n, v in sh.totals().items() if n != "calls"}
        ok = ~np.isnan(c1)
        assert np.array_equal(t["interventions"], 2 * iv1.astype(np.int64).sum(0)) and t["interventions"].dtype == np.int64
        assert np.array_equal(t["nonfinite"], 2 * np.isnan(c1).sum(0)) and t["nonfinite"].sum() == 2
        want = 2 * np.where(ok, c1.astype(np.float64), 0.0).sum(0)
        assert (np.abs(t["correction_sum"] - want) <= 1e-12 * np.abs(want)).all()
        assert np.array_equal(t["correction_max"], np.where(ok, c1, 0).max(0)) and t["correction_max"].dtype == np.float32
        assert sh.totals()["calls"] == 2
    (o1, t1, sh1), (o2, t2, _) = runs
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32))                 # bit-identical run to run, totals included
    for n in ("interventions", "nonfinite", "correction_sum", "correction_max"):
        assert torch.equal(t1[n].view(torch.uint8), t2[n].view(torch.uint8)), n
    s = sh1.summary()
    assert s["decisions"] == 2 * S.E_CASE * N and s["nonfinite"] == 2 and 0.0 < s["intervention_share"] <= 1.0
    sh1.reset_totals()
    assert all(int(v.count_nonzero()) == 0 for n, v in sh1.totals().items() if n != "calls") and sh1.calls == 0


def test_totals_over_more_envs_than_row_lanes(torch):
    """E = 2700 > 8 x 256 row lanes (strided per-lane sums: a full group of eight rows and a ragged one), N = 37: ten column tiles
    with a ragged last one."""
    from scalable_collision_avoidance_rl_amd import _native
    import ctypes as C
    E, N = 2700, 37
    rng = np.random.default_rng(2)
    iv = (rng.random((E, N)) < 0.4).astype(np.uint8)
    corr = (rng.random((E, N)) * iv).astype(np.float32)
    corr[rng.random((E, N)) < 0.05] = np.nan
    d_iv, d_c = torch.as_tensor(iv, device="cuda:0"), torch.as_tensor(corr, device="cuda:0")
    tot = [torch.zeros(N, dtype=dt, device="cuda:0") for dt in (torch.int64, torch.int64, torch.float64, torch.float32)]
    rc = _native.lib().dronesim_shield_totals(d_iv.data_ptr(), d_c.data_ptr(), E, N, *[t.data_ptr() for t in tot],
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    ok = ~np.isnan(corr)
    want = np.where(ok, corr.astype(np.float64), 0.0).sum(0)
    assert np.array_equal(host(tot[0]), iv.astype(np.int64).sum(0)) and np.array_equal(host(tot[1]), (~ok).sum(0))
    assert (np.abs(host(tot[2]) - want) <= 1e-12 * np.abs(want)).all()
    assert np.array_equal(host(tot[3]), np.where(ok, corr, 0).max(0))


# ---------------------------------------------------------------------------------------------- 4. step(execute=)
def test_step_execute_integrates_the_shielded_action_and_stores_the_nominal_one(torch):
    from scalable_collision_avoidance_rl_amd import ActionShield
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    N, E, T = 5, 16, 3
    env, twin = make_env(N, E, 21), make_env(N, E, 21)
    st = RolloutStorage(env, T)
    sh = ActionShield(env, S.RATE, S.MARGIN, S.U_MAX)
    g = torch.Generator(device="cuda:0").manual_seed(8)
    st.begin()
    changed = 0
    for t in range(T):
        nominal = torch.rand(E, N, 2, device="cuda:0", generator=g) * 3 - 1.5
        safe = sh(nominal)
        changed += int(sh.intervened.sum())
        res = env.step(nominal, into=(st, t), execute=safe)
        ref = twin.step(safe)
        assert torch.equal(st.actions[t].view(torch.int32), nominal.view(torch.int32))          # the policy's own sample
        assert torch.equal(env.pos, twin.pos) and torch.equal(env.vel, twin.vel) and torch.equal(env.vel, safe)
        assert torch.equal(res.z_states, ref.z_states) and torch.equal(env.nbr_idx, twin.nbr_idx)
        assert torch.equal(res.rewards, ref.rewards) and torch.equal(res.true_rewards, ref.true_rewards)
        assert torch.equal(res.n_collisions, ref.n_collisions) and torch.equal(res.finished, ref.finished)
    assert changed > 0
    with pytest.raises(ValueError, match="execute"):
        env.step(nominal, execute=safe.double())
    with pytest.raises(ValueError, match="execute"):
        env.step(nominal, execute=safe[:, :4])


# ---------------------------------------------------------------------------------------------- 5. closed loop
@pytest.mark.parametrize("N,k,E", [(5, 4, 64), (9, 8, 24)])
def test_closed_loop_shielded_rounds_have_no_collision(torch, N, k, E):
    """Precondition: the same env without a shield collides.  Shielded: every episode's smallest clearance >= 0.02 - 1e-5 (the
    smallest gap of the start lattice is 0.22 - 0.2; below the margin the shield lets no gap shrink).  Arrival is reported."""
    from scalable_collision_avoidance_rl_amd import ActionShield, Evaluator
    free = Evaluator(make_env(N, E, 17, k=k), "proportional", safety=True)
    clr_free = host(free.run(1)["ep_min_clearance"][0])
    env = make_env(N, E, 17, k=k)
    ev = Evaluator(env, "proportional", shield=ActionShield(env, 0.25, 0.05, 1.0, stats=True), safety=True)
    tab = ev.run(1)
    clr, coll = host(tab["ep_min_clearance"][0]), host(tab["ep_collisions"][0])
    s, ss, sf = ev.summary(), ev.safety_summary(), free.safety_summary()
    print(f"N={N} k={k} E={E}: unshielded envs with a collision {(clr_free < 0).sum()}, min clearance {clr_free.min():.4f}, arrived "
          f"{sf['arrived_share']:.3f}; shielded min clearance {clr.min():.5f}, collisions {coll.sum()}, arrived {ss['arrived_share']:.3f}, "
          f"intervention share {s['shield_intervention_share']:.4f}, mean correction {s['shield_mean_correction']:.4f}")
    assert clr_free.min() < 0
    assert (clr >= 0.02 - 1e-5).all() and coll.sum() == 0
    assert 0.0 < s["shield_intervention_share"] < 1.0 and s["shield"]["decisions"] == 200 * E * N
    # the storage holds the nominal actions: the controller's own, norm-capped at 1 and not the shielded ones
    st = ev.storage
    assert torch.equal(st.actions[0], make_twin_first_action(env, N, E, k))


def make_twin_first_action(env, N, E, k):
    twin = make_env(N, E, 17, k=k)
    twin.reset(renew_obstacles=False)                                              # the start the Evaluator's own reset drew
    return twin.control("proportional")


# ---------------------------------------------------------------------------------------------- 6. capture
def test_control_shield_step_replay_from_a_graph(torch):
    from scalable_collision_avoidance_rl_amd import ActionShield
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    N, E, T = 5, 16, 4
    sides = []
    for _ in range(2):
        env = make_env(N, E, 31, k=4)
        sides.append((env, RolloutStorage(env, T), ActionShield(env, S.RATE, S.MARGIN, S.U_MAX, stats=True), torch.zeros(E, N, 2, device="cuda:0")))

    def steps(env, st, sh, safe):
        env.reset(renew_obstacles=False)
        st.begin()
        for t in range(T):
            env.control("proportional", out=st.actions[t])
            env.step(st.actions[t], into=(st, t), execute=sh(st.actions[t], out=safe))

    for side in sides:                                                             # eager warm-up: buffers exist, counters agree
        steps(*side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        steps(*sides[1])
    for _ in range(2):
        steps(*sides[0])
        graph.replay()
        torch.cuda.synchronize()
        (ea, sa, ha, fa), (eb, sb, hb, fb) = sides
        for name in ("reward", "true_reward", "n_coll", "done", "zbuf", "nbrbuf", "actions"):
            assert torch.equal(getattr(sa, name), getattr(sb, name)), name
        assert torch.equal(ea.pos, eb.pos) and torch.equal(fa, fb)
        assert torch.equal(ha.intervened, hb.intervened) and torch.equal(ha.correction.view(torch.int32), hb.correction.view(torch.int32))
        ta, tb = ha.totals(), hb.totals()
        for n in ("interventions", "nonfinite", "correction_sum", "correction_max"):
            assert torch.equal(ta[n].view(torch.uint8), tb[n].view(torch.uint8)), n
    assert int(ha.totals()["interventions"].sum()) > 0


# ---------------------------------------------------------------------------------------------- 7. Evaluator, network actor
def test_evaluator_with_a_network_actor_and_a_shield(torch):
    from scalable_collision_avoidance_rl_amd import ActionShield, Evaluator
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    N, E = 5, 6
    env = make_env(N, E, 9)
    g = torch.Generator().manual_seed(0)
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * 0.2
    d_in = env.local_state_space
    actor = BatchedMLP(r(N, d_in, 300), r(N, 300), r(N, 300, 300), r(N, 300), r(N, 300, 16), r(N, 16), 1, 1, device="cuda:0", seed=5)
    critic = BatchedMLP(r(N, d_in, 200), r(N, 200), r(N, 200, 200), r(N, 200), r(N, 200, 1), r(N, 1), 0, 0, device="cuda:0")
    ev = Evaluator(env, actor, critic, shield=ActionShield(env, 0.25, 0.05, 1.0, stats=True), safety=True)
    tab = ev.run(2)
    assert tuple(tab["ep_len"].shape) == (2, E) and tuple(tab["agent_return"].shape) == (2, E, N)
    assert tuple(tab["mean_adv"].shape) == (2, E, N) and tuple(tab["min_clearance"].shape) == (2, E, N)
    assert tuple(tab["ep_min_clearance"].shape) == (2, E) and int(tab["collision_hist"].sum()) == 2 * E
    s = ev.summary()
    assert s["episodes"] == 2 * E and 0.0 <= s["shield_intervention_share"] <= 1.0 and s["shield_mean_correction"] >= 0.0
    assert s["shield"]["decisions"] == 2 * 200 * E * N and s["shield"]["nonfinite"] == 0
    # the storage keeps the policy's own sample: unit vectors (the discrete actor's action_index needs them)
    norm = host(ev.storage.actions).astype(np.float64)
    assert np.abs(np.linalg.norm(norm, axis=-1) - 1.0).max() <= 1e-6
    plain = Evaluator(make_env(N, E, 9), actor, critic)
    plain.run(1)
    assert "shield" not in plain.summary()
