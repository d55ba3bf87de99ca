"""GPU tests of the reward normaliser's kernels (csrc/rewnorm.hip) through `RewardNormalizer`: the running return statistics
against the float64 restatement (tests/rewnorm_ref.py) over four successive windows, the carry (window splitting), the scopes,
the map, determinism (run to run, aligned against 4-byte-offset inputs) and the exact scale equivariance.

Which shape takes which path (tests/rewnorm_ref.SHAPES):
  (7, 3, 5)     T shorter than one 8-step stage; E N = 15: the apply moves 4 bytes per lane; one ragged wave spanning 3 envs
  (33, 9, 4)    T no multiple of the stage (four full stages and one step); E N = 36 aligned: the apply's 16-byte lanes
  (17, 8, 64)   a wave's 64 columns are ONE env: the wave fetches the flags (DoneStage); two workgroups; 16-byte apply
  (40, 130, 5)  a wave spans 13 envs: every thread fetches its own flags; three workgroups, the last wave ragged; E N = 650 is
                no multiple of 4: 4-byte apply
  (5, 520, 4)   the env fold's lanes take runs of more than one env (E > 256), in `test_env_runs_longer_than_one`
  (5, 3, 300)   more agents than the group fold's 256-agent chunk, and with scope "agent" more groups than its 256 lanes, in
                `test_more_agents_than_one_chunk_of_the_group_fold`
  (16, 8192, 64) a 32 MiB window: the apply's non-temporal form, 16-byte and (offset) 4-byte, in `test_map_streams_a_large_window`
The update has NO four-columns-per-thread path in this build: one column per thread at every shape."""
import numpy as np
import pytest

from tests import rewnorm_ref as RR
from tests import test_gpu_learner as TG

pytestmark = pytest.mark.gpu
DEV = TG.DEV
SHAPE_IDS = ["x".join(map(str, s)) for s in RR.SHAPES]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def make(N, scope="team", **kw):
    from scalable_collision_avoidance_rl_amd.reward_norm import RewardNormalizer
    return RewardNormalizer(N, RR.GAMMA, DEV, scope=scope, **kw)


def dev(torch, r, d):
    return torch.from_numpy(r).to(DEV), torch.from_numpy(d).to(DEV)


def offset(torch, r):
    """The same values at an address that is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(r.numel() + 1, dtype=r.dtype, device=r.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(r.shape)
    out.copy_(r)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def check_state(norm, run, k, what=""):
    """The bars of check 1 after window k: count exact, mean within 1e-10 max|R| of the group, m2 within 1e-10 relative of the
    two-pass restatement over everything seen, scale within rtol 1e-9 of its definition ON THE STATE."""
    state, ref = norm.state.cpu().numpy(), run["twopass"][k]
    print(f"{what[:40]} window {k}: count {state[0].sum():.0f} worst mean err / max|R| {(np.abs(state[1] - ref[1]) / run['maxabs'][k]).max():.3g} "
          f"worst m2 rel err {(np.abs(state[2] - ref[2]) / ref[2]).max():.3g}")
    assert np.array_equal(state[0], ref[0]), (what, k)
    assert np.all(np.abs(state[1] - ref[1]) <= 1e-10 * run["maxabs"][k]), (what, k)
    assert np.all(np.abs(state[2] - ref[2]) <= 1e-10 * ref[2]), (what, k)
    scale = norm.scale.cpu().numpy()
    assert np.allclose(scale, RR.scale(state, norm.eps)[run["group_of"]], rtol=1e-9, atol=0), (what, k)
    for g in range(run["n_groups"]):
        assert len(set(scale[run["group_of"] == g].tolist())) == 1                               # equal within a group


def scope_of(name, N):
    return RR.two_group_map(N) if name == "map" else name


# 1, 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["team", "agent", "map"])
@pytest.mark.parametrize("shape", RR.SHAPES, ids=SHAPE_IDS)
def test_moments_carry_and_scale_over_four_windows(torch, shape, scope):
    T, E, N = shape
    scope = scope_of(scope, N)
    run = RR.run(shape, scope)
    norm = make(N, scope)
    assert norm.group_of == run["group_of"].tolist() and norm.n_groups == run["n_groups"]
    seen = 0
    for k, (r, d) in enumerate(run["windows"]):
        norm.update(*dev(torch, r, d))
        check_state(norm, run, k, f"{shape} {scope}")
        ret = norm.ret.cpu().numpy()
        assert np.all(np.abs(ret - run["ret"][k]) <= 1e-12 * run["maxabs"][k].max()), k
        assert np.array_equal(ret == 0, run["ret"][k] == 0)                                      # a reset is exactly zero
        # the NaN and inf columns take exactly the rule's steps out of the count
        seen += T * E * N - sum(RR.uncounted(T).get(k, {}).values())
        assert float(norm.count.sum()) == seen
    assert np.allclose(norm.var.cpu().numpy(), run["twopass"][3][2] / run["twopass"][3][0], rtol=1e-9)
    assert np.allclose(norm.std.cpu().numpy() * RR.scale(norm.state.cpu().numpy(), 0.0), 1.0, rtol=1e-9)


def test_env_runs_longer_than_one(torch):
    """E = 520 > the env fold's 256 lanes: runs of three envs per lane and empty lanes at the end, against the two-pass moments."""
    T, E, N = 5, 520, 4
    r, d = RR.windows(T, E, N, n=1, seed=5)[0]
    vals, ret = RR.scan(r, d, RR.GAMMA, np.zeros((E, N)))
    for scope in ("team", "agent"):
        group_of, G = RR.groups(scope, N)
        ref = RR.moments(vals, group_of, G)
        norm = make(N, scope).update(*dev(torch, r, d))
        state = norm.state.cpu().numpy()
        assert np.array_equal(state[0], ref[0])
        assert np.all(np.abs(state[1] - ref[1]) <= 1e-10 * np.abs(vals).max()) and np.all(np.abs(state[2] - ref[2]) <= 1e-10 * ref[2])
        assert np.all(np.abs(norm.ret.cpu().numpy() - ret) <= 1e-12 * np.abs(vals).max())


@pytest.mark.parametrize("scope", ["team", "agent", "map"])
def test_more_agents_than_one_chunk_of_the_group_fold(torch, scope):
    """N = 300: the group fold reads the agents' triples in two chunks, and one group per agent needs a second batch of lanes."""
    T, E, N = 5, 3, 300
    scope = scope_of(scope, N)
    group_of, G = RR.groups(scope, N)
    ws = RR.windows(T, E, N, n=2, seed=9)
    norm, ret, vals = make(N, scope), np.zeros((E, N)), []
    for r, d in ws:
        v, ret = RR.scan(r, d, RR.GAMMA, ret)
        vals.append(v)
        norm.update(*dev(torch, r, d))
    ref = RR.moments(vals, group_of, G)
    big = np.nanmax(np.where(np.isfinite(np.stack(vals)), np.abs(np.stack(vals)), 0.0))
    state = norm.state.cpu().numpy()
    assert np.array_equal(state[0], ref[0]) and state[0].sum() == 2 * T * E * N - len(RR.NAN_STEPS)
    assert np.all(np.abs(state[1] - ref[1]) <= 1e-10 * big) and np.all(np.abs(state[2] - ref[2]) <= 1e-10 * ref[2])
    assert np.allclose(norm.scale.cpu().numpy(), RR.scale(state, norm.eps)[group_of], rtol=1e-9, atol=0)
    assert np.all(np.abs(norm.ret.cpu().numpy() - ret) <= 1e-12 * big)


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RR.SHAPES, ids=SHAPE_IDS)
def test_a_window_fed_in_two_halves_is_the_same_window(torch, shape):
    """Windows 0 and 1 as one 2T window against the two fed one after the other: the test of the carry."""
    T, E, N = shape
    run = RR.run(shape, "agent")
    (r0, d0), (r1, d1) = run["windows"][:2]
    whole = make(N, "agent").update(*dev(torch, np.concatenate([r0, r1]), np.concatenate([d0, d1])))
    halves = make(N, "agent")
    halves.update(*dev(torch, r0, d0))
    halves.update(*dev(torch, r1, d1))
    assert torch.equal(whole.count, halves.count)
    for norm in (whole, halves):
        check_state(norm, run, 1, f"{shape} split")
    assert np.all(np.abs((whole.ret - halves.ret).cpu().numpy()) <= 1e-12 * run["maxabs"][1].max())


# 4 --------------------------------------------------------------------------------------------------------------------
def expected_map(torch, r, scale, clip):
    y = (r.double() * scale).float()
    if clip is not None:
        y = torch.where(y > clip, torch.full_like(y, clip), torch.where(y < -clip, torch.full_like(y, -clip), y))
    return y


def same_bits(torch, a, b):
    """NaN where the other is NaN (a NaN's payload says nothing), everywhere else the same 32 bits."""
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan])


@pytest.mark.parametrize("clip", [None, 10.0, 0.5])
@pytest.mark.parametrize("shape", RR.SHAPES, ids=SHAPE_IDS)
def test_map_is_the_scaled_reward_bit_for_bit(torch, shape, clip):
    T, E, N = shape
    run = RR.run(shape, "agent")
    norm = make(N, "agent", clip=clip)
    fresh = [dev(torch, r, d) for r, d in run["windows"]]
    for k in (RR.NAN_WINDOW, RR.INF_WINDOW):                                                      # the windows with NaN and +inf in them
        r, d = fresh[k]
        if clip is None:                                                                          # a fresh normaliser: the identity
            assert same_bits(torch, make(N, clip=None).norm(r), r)
        norm.update(r, d)
        want = expected_map(torch, r, norm.scale, clip)
        got = norm.norm(r)
        assert got.data_ptr() != r.data_ptr() and norm.norm(r).data_ptr() == got.data_ptr()       # the owned buffer, reused
        assert same_bits(torch, got, want)
        assert torch.equal(torch.isnan(got), torch.isnan(r))                                      # NaN stays NaN
        if clip is not None:
            assert float(got[~torch.isnan(got)].abs().max()) <= clip
        for src in (r, offset(torch, r)):                                                         # aligned and 4-byte-offset
            out = torch.empty_like(src)
            assert norm.norm(src, out=out) is out and same_bits(torch, out, want)
            inplace = src.clone() if src is r else offset(torch, r)
            assert norm.norm(inplace, out=inplace) is inplace and same_bits(torch, inplace, want)
        assert same_bits(torch, r, torch.from_numpy(run["windows"][k][0]).to(DEV))                                                     # the input is read only
    assert float((norm.scale - 1).abs().min()) > 0
    norm.reset()
    if clip is None:
        assert same_bits(torch, norm.norm(fresh[0][0]), fresh[0][0])                              # reset restores the identity
    assert float(norm.state.abs().sum()) == 0 and float(norm.ret.abs().sum()) == 0 and float((norm.scale - 1).abs().sum()) == 0
    # the ends of the ranges: scale 1 where the denominator is 0 (a constant return, eps = 0), not 0
    const = make(N, "team", eps=0.0, clip=None)
    z = torch.zeros(T, E, N, device=DEV)
    const.update(z, torch.ones(T, E, dtype=torch.uint8, device=DEV))
    assert float(const.count.sum()) == T * E * N and float(const.state[2].sum()) == 0 and float((const.scale - 1).abs().sum()) == 0


def test_map_streams_a_large_window(torch):
    """32 MiB: the non-temporal form of the map, with 16-byte lanes and (offset input) 4-byte lanes, out of place and in place."""
    T, E, N = 16, 8192, 64
    g = torch.Generator(device=DEV).manual_seed(3)
    r = -torch.rand(T, E, N, device=DEV, generator=g) * 300
    r[3, 5, 7] = float("nan")
    norm = make(N, "agent", clip=5.0)
    norm.scale.copy_(torch.linspace(0.01, 0.5, N, dtype=torch.float64))
    want = expected_map(torch, r, norm.scale, 5.0)
    assert same_bits(torch, norm.norm(r), want)
    off = offset(torch, r)
    assert same_bits(torch, norm.norm(off, out=off), want)
    assert same_bits(torch, norm.norm(r, out=r), want)


# 5 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RR.SHAPES, ids=SHAPE_IDS)
def test_two_runs_and_offset_inputs_give_the_same_bits(torch, shape):
    T, E, N = shape
    scope = RR.two_group_map(N)
    run = RR.run(shape, scope)
    results = []
    for variant in ("aligned", "again", "offset"):
        norm = make(N, scope)
        for r, d in run["windows"]:
            r, d = dev(torch, r, d)
            if variant == "offset":
                r = offset(torch, r)
            norm.update(r, d)
        results.append((norm.state.clone(), norm.scale.clone(), norm.ret.clone()))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)


# 6 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", ["team", "agent"])
@pytest.mark.parametrize("shape", RR.SHAPES, ids=SHAPE_IDS)
def test_scaling_the_rewards_by_a_power_of_two_changes_no_bit_of_the_normalised_rewards(torch, shape, scope):
    """eps = 0: 1024 r in place of r scales every float64 operation of the update exactly, so the scale is exactly 1 / 1024 of
    the other and the normalised rewards are bit-identical.  No tolerance."""
    T, E, N = shape
    run = RR.run(shape, scope)
    a, b = make(N, scope, eps=0.0), make(N, scope, eps=0.0)
    for r, d in run["windows"]:
        r, d = dev(torch, r, d)
        big = r * 1024
        assert same_bits(torch, big / 1024, r)
        ya, yb = a.update(r, d).norm(r).clone(), b.update(big, d).norm(big).clone()
        assert torch.equal(a.scale, b.scale * 1024) and torch.equal(a.state[0], b.state[0])
        assert torch.equal(torch.isnan(ya), torch.isnan(yb))
        assert torch.equal(torch.nan_to_num(ya, nan=0.0), torch.nan_to_num(yb, nan=0.0))
        assert float(torch.nan_to_num(ya, nan=0.0).abs().max()) > 0.1
