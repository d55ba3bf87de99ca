"""Batched policy evaluation: the reference's `benchmark_agent.py` with `TrainedAgent` (SAC_agents.py:24-124).

The reference rolls a trained actor out for 1500 episodes and logs, per episode, the reward / true reward / collisions /
length (benchmark_agent.py:59-101), the per-agent mean of ``G_t - V(z_t)`` (`benchmark_cirtic`, :104-106), the collision
histogram behind "runs with 0 collisions" (:148-156) and the running averages (:115-118).  Here:

  Evaluator      benchmark_agent.py:53-118   E envs x `rounds` fresh episodes, every env contributes exactly ONE episode per
                                             round; the per-episode tables and the histogram are reduced on the device
                                             (`dronesim_episode_eval`, `dronesim_histogram_i32`: csrc/evaluate.hip)
  TrainedAgent   SAC_agents.py:24-124        the reference class on `BatchedMLP` (network i for agent i, network 0 beyond the
                                             list; `forward`, `benchmark_cirtic`)

There is no CPU fallback: the tables come from the HIP library."""
from __future__ import annotations

import os
from collections import deque

from ._native import MAX_AGENTS as _MAX_AGENTS
from .drone_env import DONE_RADIUS

CONTROLLERS = ("proportional", "gradient")       # the commented alternatives of benchmark_agent.py:76-77
TABLES = ("ep_len", "ep_collisions", "ep_return", "ep_true_return", "agent_return", "agent_true_return", "mean_adv")
SAFETY_TABLES = ("min_clearance", "goal_dist_final", "arrive_step", "ep_min_clearance", "ep_goal_dist_max", "ep_arrived")


def episode_eval(reward, true_reward, n_coll, done, V=None, gamma=0.99, out=None, want_G=True):
    """`dronesim_episode_eval` on device tensors ``reward, true_reward [T,E,N]`` float32, ``n_coll [T,E]`` int32, ``done
    [T,E]`` uint8, ``V [T,E,N]`` float32 or None: the table of the FIRST episode of every env of the window.  Returns a dict
    of ``ep_len, ep_collisions [E]`` int32, ``ep_return, ep_true_return [E]``, ``agent_return, agent_true_return [E,N]``
    float64, ``G [T,E,N]`` float32 (`mc_returns`, bit for bit; ``want_G``) and, with ``V``, ``mean_adv [E,N]`` float64.
    ``out``: a dict of tensors to write into (the entries it lacks are not computed, except ``ep_len``)."""
    import torch
    from . import _native
    from .rollout_buffer import _prep
    reward = _prep(reward, torch.float32)
    T, E, N = reward.shape
    true_reward = _prep(true_reward, torch.float32, (T, E, N))
    n_coll = _prep(n_coll, torch.int32, (T, E))
    done = _prep(done, torch.uint8, (T, E))
    V = None if V is None else _prep(V, torch.float32, (T, E, N))
    dev = reward.device
    if out is None:
        f64 = dict(dtype=torch.float64, device=dev)
        out = dict(ep_len=torch.empty(E, dtype=torch.int32, device=dev), ep_collisions=torch.empty(E, dtype=torch.int32, device=dev),
                   ep_return=torch.empty(E, **f64), ep_true_return=torch.empty(E, **f64),
                   agent_return=torch.empty(E, N, **f64), agent_true_return=torch.empty(E, N, **f64))
        if want_G:
            out["G"] = torch.empty_like(reward)
        if V is not None:
            out["mean_adv"] = torch.empty(E, N, **f64)
    shapes = dict(ep_len=(torch.int32, (E,)), ep_collisions=(torch.int32, (E,)), ep_return=(torch.float64, (E,)),
                  ep_true_return=(torch.float64, (E,)), agent_return=(torch.float64, (E, N)),
                  agent_true_return=(torch.float64, (E, N)), mean_adv=(torch.float64, (E, N)), G=(torch.float32, (T, E, N)))
    for name, t in out.items():
        dtype, shape = shapes[name]
        if not (t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev):
            raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on {dev}")
    _native.call("dronesim_episode_eval", reward, true_reward, n_coll, done, V, float(gamma), out["ep_len"], out.get("ep_collisions"),
                 out.get("agent_return"), out.get("agent_true_return"), out.get("ep_return"), out.get("ep_true_return"), out.get("G"),
                 out.get("mean_adv"), T, E, N)
    return out


def _safety_shapes(z, nbr, done, radius, delta, z_final, nbr_final, done_radius):
    """(T, E, N, k1, c) of `episode_safety`'s arguments, or ValueError -- shapes only, nothing here touches a device."""
    import torch
    if (z_final is None) != (nbr_final is None):
        raise ValueError("z_final and nbr_final go together: the terminal observations and their neighbour lists; got only one")
    if isinstance(done_radius, bool) or not float(done_radius) == float(done_radius):
        raise ValueError(f"done_radius must be a number, got {done_radius!r}")
    if not all(torch.is_tensor(x) for x in (z, nbr, done, radius, delta)) or z.dim() != 4 or nbr.dim() != 4 or \
            tuple(nbr.shape[:3]) != tuple(z.shape[:3]):
        raise ValueError(f"z must be [T,E,N,(k+1)c] and nbr [T,E,N,k+1], got {tuple(getattr(z, 'shape', ()))} and "
                         f"{tuple(getattr(nbr, 'shape', ()))}")
    T, E, N, k1 = (int(x) for x in nbr.shape)
    if k1 < 2:
        raise ValueError(f"the neighbour lists need slot 1 (the closest neighbour): k+1 = {k1} < 2")
    c, rest = divmod(int(z.shape[3]), k1)
    if rest or c not in (2, 5):
        raise ValueError(f"z holds {int(z.shape[3])} floats per agent for {k1} rows: c must be 2 or 5")
    if not 1 <= N <= _MAX_AGENTS:
        raise ValueError(f"N must be in 1..{_MAX_AGENTS}, got {N}")
    if tuple(done.shape) != (T, E):
        raise ValueError(f"done must be [T,E] = {(T, E)}, got {tuple(done.shape)}")
    for name, x in (("radius", radius), ("delta", delta)):
        if tuple(x.shape) != (N,):
            raise ValueError(f"{name} must be [N] = ({N},), got {tuple(x.shape)}")
    if z_final is not None and not (torch.is_tensor(z_final) and torch.is_tensor(nbr_final) and tuple(z_final.shape) == tuple(z.shape)
                                    and tuple(nbr_final.shape) == tuple(nbr.shape)):
        raise ValueError(f"z_final / nbr_final must have the shapes of z / nbr, got {tuple(getattr(z_final, 'shape', ()))} and "
                         f"{tuple(getattr(nbr_final, 'shape', ()))}")
    return T, E, N, k1, c


def episode_safety(z, nbr, done, radius, delta, z_final=None, nbr_final=None, done_radius=DONE_RADIUS, out=None):
    """`dronesim_episode_safety` on device tensors: the post-step observations ``z [T,E,N,(k+1)c]`` float32 and their
    neighbour lists ``nbr [T,E,N,k+1]`` int32 (`RolloutStorage.z` / ``.nbr_idx``), ``done [T,E]`` uint8, ``radius, delta [N]``
    float32, and -- both or neither -- the terminal observations ``z_final`` / ``nbr_final`` of an auto_reset window.  The
    safety table of the FIRST episode of every env (`episode_eval`'s episode): ``ep_len [E]`` int32; ``min_clearance [E,N]``
    float32, the smallest gap to the closest neighbour, clipped at the agent's Delta; ``goal_dist_final [E,N]`` float32;
    ``arrive_step [E,N]`` int32, the first step count at which the agent stood inside its goal disk, -1 if never;
    ``ep_min_clearance``, ``ep_goal_dist_max [E]`` float32 and ``ep_arrived [E]`` uint8 over the agents.  Envs without an
    episode get NaN, -1 and 0; min / max keep a NaN.  ``out``: a dict of tensors to write into (the entries it lacks are not
    computed, except ``ep_len``; a per-env table needs the per-agent one it reduces)."""
    import torch
    from . import _native
    from .rollout_buffer import _prep
    T, E, N, k1, c = _safety_shapes(z, nbr, done, radius, delta, z_final, nbr_final, done_radius)
    z, nbr, done = _prep(z, torch.float32), _prep(nbr, torch.int32), _prep(done, torch.uint8)
    radius, delta = _prep(radius, torch.float32), _prep(delta, torch.float32)
    if z_final is not None:
        z_final, nbr_final = _prep(z_final, torch.float32), _prep(nbr_final, torch.int32)
    dev = z.device
    shapes = dict(ep_len=(torch.int32, (E,)), min_clearance=(torch.float32, (E, N)), goal_dist_final=(torch.float32, (E, N)),
                  arrive_step=(torch.int32, (E, N)), ep_min_clearance=(torch.float32, (E,)), ep_goal_dist_max=(torch.float32, (E,)),
                  ep_arrived=(torch.uint8, (E,)))
    if out is None:
        out = {name: torch.empty(shape, dtype=dtype, device=dev) for name, (dtype, shape) in shapes.items()}
    for name, t in out.items():
        dtype, shape = shapes[name]
        if not (t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev):
            raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on {dev}")
    _native.call("dronesim_episode_safety", z, nbr, z_final, nbr_final, done, radius, delta, float(done_radius), T, E, N, k1, c,
                 out["ep_len"], out.get("min_clearance"), out.get("goal_dist_final"), out.get("arrive_step"), out.get("ep_min_clearance"),
                 out.get("ep_goal_dist_max"), out.get("ep_arrived"))
    return out


def histogram_i32(values, n_bins, valid=None, out=None, accumulate=False):
    """`dronesim_histogram_i32`: ``counts[min(v, n_bins)] += 1`` over the entries of ``values`` (int32 device tensor) with
    ``v >= 0`` and ``valid != 0``; ``counts [n_bins + 1]`` int64, the last bin takes the overflow.  ``out`` / ``accumulate``:
    add into an existing table instead of writing a new one."""
    import torch
    from . import _native
    from .rollout_buffer import _prep
    values = _prep(values, torch.int32).reshape(-1)
    E = values.numel()
    if valid is not None:
        valid = valid.contiguous()
        if not (valid.device == values.device and valid.numel() == E and valid.element_size() == 1):
            raise ValueError("valid must hold one byte per value, on the values' device")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the table to add into (out=)")
        out = torch.empty(int(n_bins) + 1, dtype=torch.int64, device=values.device)
    elif not (out.dtype == torch.int64 and out.numel() == int(n_bins) + 1 and out.is_contiguous() and out.device == values.device):
        raise ValueError("out must be a contiguous int64 [n_bins + 1] tensor on the values' device")
    _native.call("dronesim_histogram_i32", values, valid, E, int(n_bins), out, 1 if accumulate else 0)
    return out


class Evaluator:
    """`benchmark_agent.py`'s loop for a batched `drones` env: ``rounds`` x E fresh episodes of an actor, no learning.

        ev = Evaluator(env, agent.actor, agent.critic)       # or Evaluator(env, "proportional")
        tables = ev.run(rounds=4)                              # device tensors, no host sync
        print(ev.summary())

    ``actor``: a `BatchedMLP` with a sampling head, or "proportional" / "gradient" (the classical baselines, one
    `rollout_control` launch per round).  ``critic``: a `BatchedMLP` value network (adds ``mean_adv``), network actors only.
    ``obs_norm``: the `ObsNormalizer` the networks were trained with -- both read ``obs_norm(env.z)``; its statistics are never
    updated here; network actors only.  ``safety=True``: a round also reduces the stored observations to the per-episode
    safety tables (`episode_safety`: closest approach, final goal distance, arrival); `safety_summary` reports them.
    ``shield``: an `ActionShield` of this env -- every action passes through it before the step integrates it, while the
    storage keeps the nominal action (``step(actions, into=, execute=safe)``).  With a controller name the round is then the
    un-fused loop ``env.control(kind)``, shield, ``step(into=, execute=)``: THREE launches per step (four with the shield's
    ``stats``); the fused `rollout_control` launch serves only without a shield.  A shield with ``stats=True`` has its
    totals cleared at the start of every ``run``, and `summary` reports its intervention share and mean correction.
    ``obstacles``: an `ObstacleField` of this env, with ``safety=True`` -- a round also reduces the stored observations to the
    per-episode obstacle tables (`obstacles.episode_obstacle_safety`: smallest gap to a disc, steps in touch with one), two
    launches more per round, and `safety_summary` gains ``obstacle_free_share``, ``arrived_clear_share``, ``min_obstacle_gap`` and
    ``mean_min_obstacle_gap``.  (Whether the discs are ENFORCED is the shield's business: ``ActionShield(env, ..., obstacles=field)``.)
    ``obstacle_inputs=True`` (network actors, with ``obstacles=field``): actor and critic read ``field.observe(env.z)``, the record
    plus the field's obstacle columns, ahead of ``obs_norm`` -- the networks of a learner with ``obstacles=field``; their ``d_in`` is
    ``field.obs_width``.  This use needs no ``safety=True`` (without it no obstacle tables are made).

    A round is ``env.reset()``, ``T = max_time_steps`` steps into an owned `RolloutStorage`, then the two reductions.  Every env
    contributes exactly one episode per round -- its first one: a fresh episode always ends inside ``max_time_steps``
    (drone_env.py:251) -- with ``auto_reset`` on or off, so short episodes are not over-represented the way they would be
    if every finished segment of a window were harvested.  Random streams are keyed by the global env id (``env.env_lo``):
    the tables of a sharded run, concatenated over the ranks, equal the single-rank run.

    Buffers are allocated by the first ``run`` (and again only when ``rounds`` changes); one round can be captured in a
    ``torch.cuda.graph`` after an eager warm-up call."""

    def __init__(self, env, actor, critic=None, gamma=0.99, n_bins=32, obs_norm=None, safety=False, shield=None, obstacles=None,
                 obstacle_inputs=False):
        from .drone_env import max_time_steps
        if not getattr(env, "batched", False):
            raise ValueError("Evaluator needs the batched (tensor) API of `drones`")
        self.env, self.gamma, self.n_bins = env, float(gamma), int(n_bins)
        if self.n_bins < 1:
            raise ValueError("n_bins < 1")
        self.controller = actor if isinstance(actor, str) else None
        if self.controller is not None:
            if actor not in CONTROLLERS:
                raise ValueError(f"actor must be a BatchedMLP or one of {CONTROLLERS}, got {actor!r}")
            if critic is not None:
                raise ValueError("a critic is evaluated along a network actor's loop; the controller rounds are one launch")
            if obs_norm is not None:
                raise ValueError("the controllers read positions, not observations: they take no obs_norm")
        else:
            if not getattr(actor, "sample_kind", 0):
                raise ValueError("the actor needs a sampling head (softmax or Gaussian BatchedMLP)")
            if obstacle_inputs:                             # the networks read the record plus the field's obstacle columns
                if getattr(obstacles, "env", None) is not env:
                    raise ValueError("obstacle_inputs=True needs obstacles=, an ObstacleField of this env")
                width, source = obstacles.obs_width, "the env with the field's obstacle columns"
            else:
                width, source = env.local_state_space, "the env"
            for net, what in ((actor, "actor"), (critic, "critic")):
                if net is not None and (net.n_agents != env.n_agents or net.d_in != width):
                    raise ValueError(f"the {what} is built for {net.n_agents} agents x {net.d_in} inputs, {source} has "
                                     f"{env.n_agents} x {width}")
            if critic is not None and critic.nout != 1:
                raise ValueError("the critic must have one output")
            if obs_norm is not None:
                obs_norm.check_networks(actor, critic)
        if obstacle_inputs and self.controller is not None:
            raise ValueError("the controllers read positions, not observations: they take no obstacle_inputs")
        self.actor, self.critic, self.obs_norm = actor, critic, obs_norm
        self.input_field = obstacles if obstacle_inputs else None      # what feeds the networks `field.observe(env.z)`
        if shield is not None and getattr(shield, "env", None) is not env:
            raise ValueError("shield must be an ActionShield of this env")
        self.shield = shield
        self.safety = bool(safety)
        if obstacles is not None:
            if getattr(obstacles, "env", None) is not env:
                raise ValueError("obstacles must be an ObstacleField of this env")
            if not self.safety and not obstacle_inputs:
                raise ValueError("the obstacle tables are part of the safety tables: obstacles= needs safety=True")
        self.obstacles = obstacles if self.safety else None             # (the field of the obstacle TABLES)
        self.obstacle_tables = None
        self.T = int(max_time_steps)
        self._rounds_run = 0
        self.storage = None
        self.tables = None
        self.safety_tables = None
        self._safe = None                                   # the shielded action of the step in flight

    def _alloc(self, rounds):
        import torch
        from .rollout_buffer import RolloutStorage
        env = self.env
        E, N, dev = env.n_envs, env.n_agents, env.device
        if self.storage is None:
            self.storage = RolloutStorage(env, self.T, actions=True, values=self.critic is not None)
            self._valid = torch.zeros(E, dtype=torch.bool, device=dev)
            self.collision_hist = torch.zeros(self.n_bins + 1, dtype=torch.int64, device=dev)
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
        t = dict(ep_len=torch.zeros(rounds, E, **i32), ep_collisions=torch.zeros(rounds, E, **i32),
                 ep_return=torch.zeros(rounds, E, **f64), ep_true_return=torch.zeros(rounds, E, **f64),
                 agent_return=torch.zeros(rounds, E, N, **f64), agent_true_return=torch.zeros(rounds, E, N, **f64))
        if self.critic is not None:
            t["mean_adv"] = torch.zeros(rounds, E, N, **f64)
        self.tables = t
        self._views = [{name: x[r] for name, x in t.items()} for r in range(rounds)]
        if self.safety:                                     # (ep_len: the same length, written by both reductions)
            f32 = dict(dtype=torch.float32, device=dev)
            s = dict(min_clearance=torch.zeros(rounds, E, N, **f32), goal_dist_final=torch.zeros(rounds, E, N, **f32),
                     arrive_step=torch.zeros(rounds, E, N, **i32), ep_min_clearance=torch.zeros(rounds, E, **f32),
                     ep_goal_dist_max=torch.zeros(rounds, E, **f32), ep_arrived=torch.zeros(rounds, E, dtype=torch.uint8, device=dev))
            self.safety_tables = s
            self._safety_views = [dict({name: x[r] for name, x in s.items()}, ep_len=t["ep_len"][r]) for r in range(rounds)]
        if self.obstacles is not None:
            f32 = dict(dtype=torch.float32, device=dev)
            o = dict(min_obstacle_gap=torch.zeros(rounds, E, N, **f32), obstacle_hit_steps=torch.zeros(rounds, E, N, **i32),
                     ep_min_obstacle_gap=torch.zeros(rounds, E, **f32), ep_obstacle_hit_steps=torch.zeros(rounds, E, **i32))
            self.obstacle_tables = o
            self._obstacle_views = [dict({name: x[r] for name, x in o.items()}, ep_len=t["ep_len"][r]) for r in range(rounds)]

    def rollout(self):
        """One round's experience: ``env.reset()`` and ``T`` steps into ``self.storage`` (no reduction)."""
        env, st = self.env, self.storage
        env.reset(renew_obstacles=False)                                        # benchmark_agent.py:112
        shield = self.shield
        if self.controller is not None:
            if shield is None:
                env.rollout_control(self.controller, self.T, record_actions=True, into=st)
                return st
            if self._safe is None:
                self._safe = st.actions[0].clone()
            st.begin()
            for t in range(self.T):                                             # control, shield, step: three launches per step
                env.control(self.controller, out=st.actions[t])
                env.step(st.actions[t], into=(st, t), execute=shield(st.actions[t], out=self._safe))
            return st
        actor, critic, norm, field = self.actor, self.critic, self.obs_norm, self.input_field
        st.begin()
        for t in range(self.T):                                                 # :69-94
            z = env.z if field is None else field.observe(env.z)                # raw -> obstacle columns -> normaliser
            z = z if norm is None else norm(z)                                  # (the statistics are never updated here)
            if critic is not None:
                critic.forward(z, out=st.values[t])
            actor.sample_action(z, env=env, act_out=st.actions[t])              # :78
            if shield is None:
                env.step(st.actions[t], into=(st, t))                           # :81-83
            else:                                                               # the storage keeps the policy's own sample
                if self._safe is None:
                    self._safe = st.actions[0].clone()
                env.step(st.actions[t], into=(st, t), execute=shield(st.actions[t], out=self._safe))
        return st

    def run(self, rounds=1):
        """``rounds`` x E episodes.  Returns a dict of device tensors (the same objects on every call): ``ep_len``,
        ``ep_collisions`` int32 and ``ep_return``, ``ep_true_return`` float64 ``[rounds, E]`` (benchmark_agent.py:98-101),
        ``agent_return``, ``agent_true_return`` and -- with a critic -- ``mean_adv`` float64 ``[rounds, E, N]`` (:104-106),
        ``collision_hist`` int64 ``[n_bins + 1]`` over all rounds of this call (:148-156; the last bin holds the episodes with
        ``n_bins`` collisions or more).  With ``safety=True`` also the tables of `episode_safety` (`SAFETY_TABLES`) as
        ``[rounds, E(, N)]`` tensors, one more call per round, and with ``obstacles=`` the obstacle tables
        (`obstacles.OBSTACLE_TABLES`) likewise.  No host synchronisation."""
        import torch
        rounds = int(rounds)
        if rounds < 1:
            raise ValueError("rounds < 1")
        if self.tables is None or self.tables["ep_len"].shape[0] != rounds:
            self._alloc(rounds)
        self._rounds_run = rounds
        if self.shield is not None and self.shield.stats:
            self.shield.reset_totals()
        for r in range(rounds):
            st = self.rollout()
            out = self._views[r]
            episode_eval(st.reward, st.true_reward, st.n_coll, st.done, st.values if self.critic is not None else None,
                         self.gamma, out=out)
            torch.ne(out["ep_len"], 0, out=self._valid)
            histogram_i32(out["ep_collisions"], self.n_bins, valid=self._valid, out=self.collision_hist, accumulate=r > 0)
            if self.safety:
                st.safety(out=self._safety_views[r])
            if self.obstacles is not None:
                self.obstacles.episode_safety(st, out=self._obstacle_views[r])
        if self.obstacles is not None:
            return dict(self.tables, collision_hist=self.collision_hist, **self.safety_tables, **self.obstacle_tables)
        if self.safety:
            return dict(self.tables, collision_hist=self.collision_hist, **self.safety_tables)
        return dict(self.tables, collision_hist=self.collision_hist)

    # fixed-length float64 vector of one rank: [episodes, sum return, sum true return, sum collisions, sum length,
    # episodes without a collision, histogram (n_bins + 1), per-agent sum of mean_adv (N)]
    def _vector(self):
        import torch
        t = self.tables
        if t is None:
            raise RuntimeError("run() first")
        ok = t["ep_len"] > 0
        f = lambda x: (x.double() * ok).sum().view(1)
        adv = ((t["mean_adv"] * ok[..., None]).sum((0, 1)) if "mean_adv" in t
               else torch.zeros(self.env.n_agents, dtype=torch.float64, device=ok.device))
        return torch.cat([ok.sum().double().view(1), f(t["ep_return"]), f(t["ep_true_return"]), f(t["ep_collisions"]), f(t["ep_len"]),
                          (ok & (t["ep_collisions"] == 0)).sum().double().view(1), self.collision_hist.double(), adv])

    def summary(self, group=None):
        """Host-side figures of the last ``run`` (benchmark_agent.py:115-120, :151): episodes, mean return / true return /
        collisions / length per episode, the share of episodes with 0 collisions, the histogram and the per-agent mean
        advantage; with a shield that keeps ``stats``, also ``shield_intervention_share`` and ``shield_mean_correction`` (and the
        shield's whole `ActionShield.summary` under ``shield``).  With ``torch.distributed`` initialised, ONE all-gather of this rank's fixed-length float64 vector
        (`sharding.all_gather_stats`) makes the figures global, the same on every rank."""
        from .sharding import all_gather_stats
        out = summarize_evaluation(all_gather_stats(self._vector(), group), self.n_bins, self.critic is not None)
        if self.shield is not None and self.shield.stats:   # (this rank's shield: its totals are not gathered)
            s = self.shield.summary(calls=self._rounds_run * self.T)
            out["shield_intervention_share"], out["shield_mean_correction"] = s["intervention_share"], s["mean_correction"]
            out["shield"] = s
        return out


    # fixed-length float64 vector of one rank: [episodes, arrived, successes, sum ep_min_clearance, min ep_min_clearance (+inf
    # without an episode), sum ep_goal_dist_max, agents that arrived, sum of their arrive_step]; with an obstacle field four more:
    # [episodes without an obstacle hit, arrived with no collision and no hit, sum ep_min_obstacle_gap, min ep_min_obstacle_gap]
    def _safety_vector(self):
        import torch
        t, s = self.tables, self.safety_tables
        if not self.safety:
            raise RuntimeError("safety_summary needs Evaluator(..., safety=True)")
        if t is None or s is None:
            raise RuntimeError("run() first")
        ok = t["ep_len"] > 0
        zero, inf = torch.zeros((), dtype=torch.float64, device=ok.device), torch.full((), float("inf"), dtype=torch.float64, device=ok.device)
        arrived = ok & (s["ep_arrived"] != 0)
        clr, goal = s["ep_min_clearance"].double(), s["ep_goal_dist_max"].double()
        there = ok[..., None] & (s["arrive_step"] > 0)
        cnt = lambda m: m.sum().double().view(1)
        v = [cnt(ok), cnt(arrived), cnt(arrived & (t["ep_collisions"] == 0)), torch.where(ok, clr, zero).sum().view(1),
             torch.where(ok, clr, inf).min().view(1), torch.where(ok, goal, zero).sum().view(1), cnt(there),
             torch.where(there, s["arrive_step"].double(), zero).sum().view(1)]
        if self.obstacles is not None:                      # four more: see `summarize_safety`
            o = self.obstacle_tables
            free = ok & (o["ep_obstacle_hit_steps"] == 0)
            gap = o["ep_min_obstacle_gap"].double()
            v += [cnt(free), cnt(arrived & (t["ep_collisions"] == 0) & free), torch.where(ok, gap, zero).sum().view(1),
                  torch.where(ok, gap, inf).min().view(1)]
        return torch.cat(v)

    def safety_summary(self, group=None):
        """Host-side safety figures of the last ``run`` of an ``Evaluator(..., safety=True)``: episodes, the share that arrived
        (every agent inside its goal disk at the end), the share of successes (arrived without a collision), mean and minimum
        of the episodes' smallest clearance, the mean of their largest final goal distance, the mean step count at which an
        agent that arrived first stood inside its goal disk.  With ``obstacles=``: ``obstacle_free_share`` (episodes in which no
        agent touched a disc), ``arrived_clear_share`` (arrived with no collision and no obstacle hit), ``min_obstacle_gap`` and
        ``mean_min_obstacle_gap`` over the episodes' smallest gaps.  ONE all-gather of a fixed-length vector, as `summary`."""
        from .sharding import all_gather_stats
        return summarize_safety(all_gather_stats(self._safety_vector(), group))


def summarize_safety(gathered):
    """`Evaluator.safety_summary` from the gathered ``[world, 8]`` vectors -- ``[world, 12]`` with an obstacle field: episodes
    without an obstacle hit, arrived with no collision and no hit, sum and minimum of the episodes' smallest obstacle gap --
    (host side): sums over the ranks, except the smallest clearance and the smallest obstacle gap, which are minima over them."""
    g = gathered.double().cpu()
    if g.shape[1] not in (8, 12):
        raise ValueError(f"the safety vectors hold 8 figures, 12 with an obstacle field, got {g.shape[1]}")
    tot = g.sum(0)
    n, eps, agents = int(tot[0]), max(float(tot[0]), 1.0), float(tot[6])
    out = {"episodes": n, "arrived_share": float(tot[1]) / eps, "success_share": float(tot[2]) / eps,
           "mean_min_clearance": float(tot[3]) / eps, "min_clearance": float(g[:, 4].min()) if n else None,
           "mean_goal_dist_max": float(tot[5]) / eps, "mean_arrive_step": float(tot[7]) / agents if agents else None,
           "world_size": int(gathered.shape[0])}
    if g.shape[1] == 12:
        out.update(obstacle_free_share=float(tot[8]) / eps, arrived_clear_share=float(tot[9]) / eps,
                   min_obstacle_gap=float(g[:, 11].min()) if n else None, mean_min_obstacle_gap=float(tot[10]) / eps)
    return out


def summarize_evaluation(gathered, n_bins, has_critic=True):
    """`Evaluator.summary` from the gathered ``[world, 6 + n_bins + 1 + N]`` vectors (host side)."""
    tot = gathered.double().sum(0).cpu()
    eps = max(float(tot[0]), 1.0)
    hist = [int(x) for x in tot[6:6 + n_bins + 1]]
    out = {"episodes": int(tot[0]), "mean_return": float(tot[1]) / eps, "mean_true_return": float(tot[2]) / eps,
           "mean_collisions": float(tot[3]) / eps, "mean_length": float(tot[4]) / eps, "zero_collision_share": float(tot[5]) / eps,
           "collision_hist": hist, "world_size": int(gathered.shape[0])}
    out["mean_advantage"] = [float(x) / eps for x in tot[6 + n_bins + 1:]] if has_critic else None
    return out


def network_index(n_networks, n_agents, only_one_NN=False):
    """Which saved network serves agent i: network i while ``i < n_networks``, otherwise network 0 (SAC_agents.py:72-75,
    :93-96); ``only_one_NN``: network 0 for every agent (:88-92)."""
    if n_networks < 1:
        raise ValueError("an empty list of networks")
    return [0 if only_one_NN or i >= n_networks else i for i in range(int(n_agents))]


class TrainedAgent:
    """The reference's `TrainedAgent` (SAC_agents.py:24-124) on `BatchedMLP`: loads the saved critics and actors
    (``models_dir/critics_name``, ``models_dir/actors_name``; `compat.load_reference_modules`, the reference's code is not
    needed) and stacks them per agent -- network i for agent i, network 0 beyond the end of a list.  ``n_agents="auto"``
    takes the number of critics (:41-44).  ``.actor`` / ``.critic`` are the stacked `BatchedMLP`s (they plug into `Evaluator`),
    ``**mlp_kw`` goes to their constructor (``precision=``, ``seed=``, ``device=``).  A missing file raises
    ``FileNotFoundError`` (the reference prints and exits)."""

    def __init__(self, critics_name: str, actors_name: str, n_agents="auto", discount=0.99, models_dir="models", **mlp_kw):
        from .compat import load_reference_modules
        critics = load_reference_modules(os.path.join(models_dir, critics_name))
        actors = load_reference_modules(os.path.join(models_dir, actors_name))
        self.critics_name, self.actors_name = critics_name, actors_name
        self._init(critics, actors, n_agents, discount, mlp_kw)

    @classmethod
    def from_modules(cls, critics, actors, n_agents="auto", discount=0.99, **mlp_kw):
        """The same agent from in-memory lists of networks (anything with the reference's attribute names)."""
        self = cls.__new__(cls)
        self.critics_name = self.actors_name = None
        self._init(list(critics), list(actors), n_agents, discount, mlp_kw)
        return self

    def _init(self, critics, actors, n_agents, discount, mlp_kw):
        from .policies import BatchedMLP, stack_reference_modules
        self.criticsNN, self.actors = critics, actors
        self.n_agents = len(critics) if n_agents == "auto" else int(n_agents)          # :41-44
        self.discount = discount                                                         # :58
        self._mlp_kw = dict(mlp_kw)
        self.actor_index = network_index(len(actors), self.n_agents)
        self.critic_index = network_index(len(critics), self.n_agents)
        critic_kw = {k: v for k, v in mlp_kw.items() if k != "seed"}
        self.actor = BatchedMLP(*stack_reference_modules([actors[j] for j in self.actor_index]), **mlp_kw)
        self.critic = BatchedMLP(*stack_reference_modules([critics[j] for j in self.critic_index], "critic"), **critic_kw)
        self._critic0 = None

    def _critic_for(self, only_one_NN):
        if not only_one_NN:
            return self.critic
        if self._critic0 is None:
            from .policies import BatchedMLP, stack_reference_modules
            kw = {k: v for k, v in self._mlp_kw.items() if k != "seed"}
            self._critic0 = BatchedMLP(*stack_reference_modules([self.criticsNN[0]] * self.n_agents, "critic"), **kw)
        return self._critic0

    def forward(self, z_states: list, N: list = None):
        """``actions = agents.forward(z_states, Ni)`` of the E = 1 face (:60-82): a list of ``n_agents`` actions ``[2]``."""
        import numpy as np
        import torch
        z = np.stack([np.asarray(z_states[i], np.float64).reshape(-1) for i in range(self.n_agents)])
        act, _ = self.actor.sample_action(torch.as_tensor(z[None], dtype=torch.float32))
        a = act[0].double().cpu().numpy()
        return [a[i] for i in range(self.n_agents)]

    def benchmark_cirtic(self, buffers, only_one_NN=False):
        """``(Gts, V_approxs)`` as the reference returns them (:84-124): per agent, the Monte-Carlo returns of the stored
        rewards (float64 ``[T]``) and the critic's values of the stored states (float32 ``[T]``).  ``buffers``: the
        reference's `ExperienceBuffers` (anything with ``.buffers[i][t].z_state`` / ``.reward``) or a `RolloutStorage` --
        then the returns restart at every ``done`` and the arrays are ``[T, E]`` (``[T]`` at E = 1).  Both run on the
        device (`dronesim_returns`, the batched critic)."""
        import numpy as np
        import torch
        from .rollout_buffer import mc_returns
        critic = self._critic_for(only_one_NN)
        dev, n = critic.device, self.n_agents
        if hasattr(buffers, "buffers"):
            states = np.stack([np.stack([np.asarray(x.z_state, np.float64).reshape(-1) for x in buffers.buffers[i]]) for i in range(n)], 1)
            rewards = np.stack([np.asarray([float(x.reward) for x in buffers.buffers[i]]) for i in range(n)], 1)
            z = torch.as_tensor(states, dtype=torch.float32, device=dev)                          # [T, N, d]
            reward = torch.as_tensor(rewards, dtype=torch.float32, device=dev).unsqueeze(1)       # [T, 1, N]
            done = None
        else:
            z, reward, done = buffers.z_pre.reshape(-1, n, critic.d_in), buffers.reward, buffers.done
        T, E = reward.shape[:2]
        G = mc_returns(reward, self.discount, done).double().cpu().numpy()                        # :107-113
        V = critic.forward(z).reshape(T, E, n).cpu().numpy()                                      # :118
        sq = (lambda a: a[:, 0]) if E == 1 else (lambda a: a)
        return deque(sq(G[:, :, i]) for i in range(n)), deque(sq(V[:, :, i]) for i in range(n))

    benchmark_critic = benchmark_cirtic
