"""Action shield: a local collision-avoidance filter between the policy and ``env.step()``.

The reference's only collision avoidance is the log barrier in the reward (drone_env.py:309-332); a trained or classical action
goes into ``step()`` unchanged.  The shield replaces the nominal action of every agent by the closest action (Euclidean
projection) that does not close the gap to any neighbour of its OWN observation faster than ``rate`` of that gap per step, inside
the per-component box ``u_max``.  Everything it reads is what the agent acts on: rows 1..k of its ``z`` record (``x_j - x_i`` of
the k closest agents inside Delta), ``nbr_idx`` (ids outside ``[0, N)`` are ghost rows), the radii and the single-integrator
dynamics ``x' = x + dt u`` (drone_env.py:78-79, 235).  The rule (include/dronesim.h states it for the kernel, tests/shield_ref.py
in float64) -- half-planes ``a.x <= b`` in this order:

  1. the box ``(+1,0), (-1,0), (0,+1), (0,-1)`` with ``b = u_max`` (``+inf``: never binds);
  2. slot ``s = 1..k``, ``j = nbr[s]``, ``p`` = floats 0, 1 of row ``s``, ``d = |p|``: skipped unless ``0 <= j < N``, ``j != i``,
     ``d`` finite and ``> 0``; otherwise ``a = p / d``, ``g = d - radius[i] - radius[j] - margin``, ``b = rate max(g, 0) / dt``.

Where two agents list each other and both are shielded with the same ``rate <= 1/2`` and ``margin``, the gap after the step is at
least ``(1 - 2 rate) g`` where ``g >= 0`` and does not shrink where ``g < 0`` (DESIGN.md has the argument and the conditions: agents
outside the list are unconstrained, so Delta must exceed ``2 sqrt(2) u_max dt + margin``, and with ``k`` below the local crowd the
shield reduces collisions but does not exclude them).

With ``obstacles=field`` (an `obstacles.ObstacleField` of the env) the set also holds one half-plane per disc of the agent's obstacle
list, behind the neighbour slots: slot ``s`` of ``field.sense(z)``, skipped where empty; ``a = row.xy / d``,
``g = d - radius[i] - row.r - margin``, ``b = obstacle_rate max(g, 0) / dt``.  A disc does not move, so the agent may spend the whole
budget: ``obstacle_rate`` in (0, 1], default ``rate``.  For a listed disc the gap after the step is at least
``(1 - obstacle_rate) g`` where ``g >= 0`` and does not shrink where ``g < 0`` (the range must exceed
``sqrt(2) u_max dt + margin``; with more than ``m`` discs in range hits become rarer, not impossible).

  ActionShield   one `dronesim_action_shield` launch per call (csrc/shield.hip), one `dronesim_shield_totals` more with ``stats``;
                 with ``obstacles=``: `dronesim_obstacle_sense`, then `dronesim_action_shield_obstacles` (two launches, three with
                 ``stats``)

There is no CPU fallback; importing this module needs neither a GPU nor the library."""
from __future__ import annotations

import math

from ._native import MAX_AGENTS as _MAX_AGENTS, MAX_K as _MAX_K, check_tensor as _check_tensor


def _number(name, x):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or x != x:
        raise ValueError(f"{name} must be a number, got {x!r}")
    return float(x)


def check_shield_params(rate, margin, u_max):
    """``(rate, margin, u_max)`` as floats (``u_max=None`` -> ``+inf``, no box), or ValueError: ``rate`` in (0, 0.5], ``margin``
    finite and >= 0, ``u_max`` > 0."""
    rate, margin = _number("rate", rate), _number("margin", margin)
    u_max = math.inf if u_max is None else _number("u_max", u_max)
    if not 0.0 < rate <= 0.5:
        raise ValueError(f"rate must be in (0, 0.5] (two agents that face each other each take at most `rate` of the gap), got {rate}")
    if not 0.0 <= margin < math.inf:
        raise ValueError(f"margin must be finite and >= 0, got {margin}")
    if not u_max > 0.0:
        raise ValueError(f"u_max must be > 0 (None or +inf: no box), got {u_max}")
    return rate, margin, u_max


def check_obstacle_rate(obstacle_rate, rate):
    """``obstacle_rate`` as a float in (0, 1] (``None`` -> ``rate``), or ValueError."""
    if obstacle_rate is None:
        return rate
    obstacle_rate = _number("obstacle_rate", obstacle_rate)
    if not 0.0 < obstacle_rate <= 1.0:
        raise ValueError(f"obstacle_rate must be in (0, 1] (a disc does not move: the agent may take the whole gap), got {obstacle_rate}")
    return obstacle_rate


def _shield_shapes(actions, z, nbr, out, radius, E, N, k1, c, device):
    """ValueError unless the arguments of `ActionShield.shield` are what the launch reads -- shapes, dtypes and devices only,
    nothing here touches a device."""
    import torch
    if not 1 <= N <= _MAX_AGENTS or not 2 <= k1 <= _MAX_K + 1 or c not in (2, 5):
        raise ValueError(f"the shield needs N in 1..{_MAX_AGENTS}, k + 1 in 2..{_MAX_K + 1} and c in (2, 5), got N = {N}, k + 1 = {k1}, c = {c}")
    want = (("actions", actions, torch.float32, (E, N, 2)), ("z", z, torch.float32, (E, N, k1 * c)), ("nbr", nbr, torch.int32, (E, N, k1)),
            ("radius", radius, torch.float32, (N,)))
    if out is not None:
        want += (("out", out, torch.float32, (E, N, 2)),)
    for name, x, dtype, shape in want:
        _check_tensor(name, x, dtype, shape, device)


class ActionShield:
    """The shield of a batched `drones` env.

        shield = ActionShield(env, rate=0.25, margin=0.05, u_max=1.0, stats=True)
        safe = shield(actions)                                  # [E,N,2]; reads env.z, env.nbr_idx, the env's radii and dt
        env.step(actions, into=(storage, t), execute=safe)      # the storage keeps the policy's own sample

    ``shield(actions, z=None, nbr=None, out=None)``: ``z`` / ``nbr`` default to the env's current observation (any observation of
    the env's shape serves, e.g. a `RolloutStorage` ring slot); ``out`` may be ``actions`` itself.  ``intervened`` (uint8) and
    ``correction`` (float32, ``|u* - u|``; NaN where the action was not finite and went through unchanged) ``[E,N]`` hold the
    last call's planes.  ``stats=True`` adds one launch per call that folds them into per-agent running totals
    (`totals`, `reset_totals`).  Buffers are allocated by the first call; after an eager warm-up the calls can be captured in a
    ``torch.cuda.graph``.  Shape, dtype and device mistakes raise ValueError before anything touches a device.

    ``obstacles``: an `ObstacleField` of this env -- every call then senses the field from the same ``z`` and adds the listed
    discs' half-planes with ``obstacle_rate`` (default ``rate``); ``None``: the plain launch, today's bits."""

    def __init__(self, env, rate=0.25, margin=0.0, u_max=None, stats=False, obstacles=None, obstacle_rate=None):
        if not getattr(env, "batched", False):
            raise ValueError("ActionShield needs the batched (tensor) API of `drones`")
        self.rate, self.margin, self.u_max = check_shield_params(rate, margin, u_max)
        if obstacles is None and obstacle_rate is not None:
            raise ValueError("obstacle_rate needs obstacles= (an ObstacleField of this env)")
        if obstacles is not None and getattr(obstacles, "env", None) is not env:
            raise ValueError("obstacles must be an ObstacleField of this env")
        self.obstacles = obstacles
        self.obstacle_rate = None if obstacles is None else check_obstacle_rate(obstacle_rate, self.rate)
        self.env, self.stats = env, bool(stats)
        self.intervened = self.correction = None
        self._totals = None
        self.calls = 0

    def _alloc(self):
        import torch
        env = self.env
        E, N, dev = env.n_envs, env.n_agents, env.device
        self.intervened = torch.zeros(E, N, dtype=torch.uint8, device=dev)
        self.correction = torch.zeros(E, N, dtype=torch.float32, device=dev)
        if self.stats:
            self._totals = dict(interventions=torch.zeros(N, dtype=torch.int64, device=dev),
                                nonfinite=torch.zeros(N, dtype=torch.int64, device=dev),
                                correction_sum=torch.zeros(N, dtype=torch.float64, device=dev),
                                correction_max=torch.zeros(N, dtype=torch.float32, device=dev))

    def shield(self, actions, z=None, nbr=None, out=None):
        """The shielded actions ``[E,N,2]`` of the nominal ``actions`` (a new tensor, or ``out``)."""
        import torch
        from . import _native
        from .drone_env import dt
        env = self.env
        E, N, k1, c = env.n_envs, env.n_agents, env.k_closest + 1, env.c
        z = env.z if z is None else z
        nbr = env.nbr_idx if nbr is None else nbr
        radius = env._radius
        _shield_shapes(actions, z, nbr, out, radius, E, N, k1, c, env.device)
        if self.intervened is None:
            self._alloc()
        if out is None:
            out = torch.empty_like(actions)
        field = self.obstacles
        if field is not None:                               # the agent's obstacle list, from the observation it acts on
            orow, oid = field.sense(z)
        shared = (z, nbr, actions, radius, self.rate, self.margin, self.u_max, dt, E, N, k1, c, out, self.intervened, self.correction)
        if field is None:
            _native.call("dronesim_action_shield", *shared)
        else:
            _native.call("dronesim_action_shield_obstacles", *shared, orow, oid, field.m, field.M, self.obstacle_rate)
        if self.stats:
            t = self._totals
            _native.call("dronesim_shield_totals", self.intervened, self.correction, E, N, t["interventions"], t["nonfinite"],
                         t["correction_sum"], t["correction_max"])
        self.calls += 1
        return out

    __call__ = shield

    def totals(self):
        """The running totals since the last `reset_totals`, per agent, as device tensors (the same objects on every call):
        ``interventions``, ``nonfinite`` int64 ``[N]``, ``correction_sum`` float64 and ``correction_max`` float32 ``[N]`` over the
        finite actions, and ``calls`` (host int: ``calls * E`` decisions per agent)."""
        if not self.stats:
            raise RuntimeError("totals needs ActionShield(..., stats=True)")
        if self._totals is None:
            self._alloc()
        return dict(self._totals, calls=self.calls)

    def reset_totals(self):
        if not self.stats:
            raise RuntimeError("reset_totals needs ActionShield(..., stats=True)")
        if self._totals is not None:
            for t in self._totals.values():
                t.zero_()
        self.calls = 0

    def summary(self, calls=None):
        """Host-side figures of the totals (one device read): the share of (call, env, agent) decisions the shield changed, the
        mean correction over ALL finite decisions and over the changed ones, the largest correction, the non-finite actions.
        ``calls``: the calls the totals hold, where the host's own count does not know them (replays of a captured graph add to
        the device totals, not to ``self.calls``)."""
        import torch
        t = self.totals()
        calls = self.calls if calls is None else int(calls)
        v = torch.cat([t["interventions"].double().sum().view(1), t["nonfinite"].double().sum().view(1),
                       t["correction_sum"].sum().view(1), t["correction_max"].double().max().view(1)]).cpu()
        n, nan = float(v[0]), float(v[1])
        decisions = float(calls) * self.env.n_envs * self.env.n_agents
        finite = max(decisions - nan, 1.0)
        return {"decisions": int(decisions), "intervention_share": n / max(decisions, 1.0), "mean_correction": float(v[2]) / finite,
                "mean_correction_intervened": float(v[2]) / n if n else 0.0, "max_correction": float(v[3]), "nonfinite": int(nan)}
