"""Static obstacle discs that matter: sensing, and per-episode clearance / hit tables.

The reference draws ``n_obstacles`` discs ``[x, y, r]`` and only paints them (drone_env.py:155-169: "never read by dynamics or
reward"), and so does `drones`.  This module makes them real in the layers that handle safety, beside the step -- the step kernel,
the does not change, and the reward and the networks' input change only where `observe` / `shape_reward` are asked for:

  ObstacleField.observe          `dronesim_obstacle_observe`: every record with its obstacle columns -- the list below as ``(p.x, p.y,
                                 r)`` per slot -- the input of obstacle-aware networks (``obs_width`` floats per agent)
  ObstacleField.shape_reward     `dronesim_obstacle_reward`: the obstacle cost of the observation after every stored step, taken
                                 off its reward; ``SA2CLearner`` / ``PPOLearner(obstacles=field, obstacle_weight=w)`` use both
  ObstacleField.sense           `dronesim_obstacle_sense` (csrc/obstacles.hip): per agent, the ``m`` nearest discs within its range,
                                 from its OWN observation (row 0 is ``x_i - xF_i``, so the record holds the position)
  ActionShield(obstacles=field)  one half-plane per listed disc in the projection (shield.py, csrc/shield.hip)
  ObstacleField.episode_safety   `dronesim_episode_obstacle_safety`: clearance and hit tables of every env's first episode from a
                                 stored window; ``Evaluator(..., safety=True, obstacles=field)`` reports them
  place_obstacles                host numpy: discs of the reference's sizes that leave given points (the goals) free
  ObstacleField(per_env=True)    a disc list PER ENV, ``[E,M,3]`` with ``counts [E]``: the same four methods on the
                                 `dronesim_env_obstacle_*` entries (csrc/env_obstacles.hip, include/dronesim_env_obstacles.h)
  place_obstacles_per_env        `place_obstacles` per env, seeded ``[seed, e]``, zero-padded to one width

The rule (include/dronesim.h states it for the kernels, tests/obstacle_ref.py in float64): ``x = z[0] + xF[i][0]``,
``y = z[1] + xF[i][1]``; to disc ``o``: ``p = o.xy - (x, y)``, ``d = |p|``, ``gap = d - radius[i] - o.r``.  A disc is in range where
``gap <= sense[i]``; the list holds the ``m`` smallest gaps, ties to the lower id; ``gap_min`` / ``hit`` cover ALL discs.  The
obstacle cost is the reference's collision term with a disc in the neighbour's place: over ALL discs ``9.99e3`` where ``gap <= 0``,
``log(sense[i] / gap)`` where ``0 < gap <= sense[i]``, 0 otherwise, times a weight (tests/obstacle_obs_ref.py restates it).

Without ``per_env`` one list ``[M,3]`` serves all envs.  ``env.reset(renew_obstacles=True)`` (the reference's default) redraws
``env.obstacles``; a field follows only through ``field.set(env.obstacles)``.  With ``per_env=True`` every env senses, avoids and
pays for its OWN discs: ``obstacles [E,M,3]`` (``M <= 64``), env ``e`` holding rows ``0..counts[e]-1``, ids env-local; the rule is
the same with env ``e``'s list in place of the shared one, and the outputs are bit-identical to the shared kernels run on that
env's records with that env's list.  ``field.set(*place_obstacles_per_env(..., seed=window))`` between windows redraws them the way
the reference's ``reset()`` does; inside a stored window a list does not change (the tables and the shaped reward read one list per
env for the whole window).  The shield, the `Evaluator` and the learners work through the field and need nothing else.

There is no CPU fallback; importing this module needs neither a GPU nor the library."""
from __future__ import annotations

import numpy as np

from ._native import (MAX_AGENTS as _MAX_AGENTS, MAX_ENV_OBSTACLES, MAX_K as _MAX_K, MAX_OBSTACLES, MAX_SENSE,
                      check_tensor as _tensor_check)

OBSTACLE_TABLES = ("min_obstacle_gap", "obstacle_hit_steps", "ep_min_obstacle_gap", "ep_obstacle_hit_steps")


def check_obstacles(obstacles, M=None):
    """``obstacles`` as a float64 ``[M,3]`` array (x, y, r), or ValueError: wrong shape, non-finite entries, ``r < 0``, more than
    `MAX_OBSTACLES` discs, or -- with ``M`` -- another count than ``M``."""
    try:
        obs = np.array(obstacles, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"obstacles must be an [M,3] array of (x, y, r), got {type(obstacles).__name__}") from None
    if obs.ndim == 1 and obs.size == 0:                        # (an empty list)
        obs = obs.reshape(0, 3)
    if obs.ndim != 2 or obs.shape[1] != 3:
        raise ValueError(f"obstacles must be an [M,3] array of (x, y, r), got shape {obs.shape}")
    if obs.shape[0] > MAX_OBSTACLES:
        raise ValueError(f"at most {MAX_OBSTACLES} obstacles (the list is staged per workgroup), got M = {obs.shape[0]}")
    if not np.isfinite(obs).all():
        raise ValueError("obstacles must be finite")
    if (obs[:, 2] < 0).any():
        raise ValueError("obstacle radii must be >= 0")
    if M is not None and obs.shape[0] != M:
        raise ValueError(f"M is fixed at construction: this field holds {M} obstacles, got {obs.shape[0]}")
    return obs


def check_env_obstacles(obstacles, counts=None, E=None, M=None):
    """Per-env lists: ``obstacles`` as a float64 ``[E,M,3]`` array (x, y, r) and ``counts`` as an int64 ``[E]`` array (default: all
    ``M``), or ValueError: wrong rank or shape, ``M > MAX_ENV_OBSTACLES``, non-finite entries or ``r < 0`` in ANY row (the rows
    behind an env's count are padding, but they are uploaded), counts that are no integers in ``0..M``, or -- with ``E`` / ``M`` --
    another env count / row count than those.  Nothing here touches a device."""
    try:
        obs = np.array(obstacles, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"per-env obstacles must be an [E,M,3] array of (x, y, r), got {type(obstacles).__name__}") from None
    if obs.ndim != 3 or obs.shape[2] != 3:
        raise ValueError(f"per-env obstacles must be an [E,M,3] array of (x, y, r), got shape {obs.shape}")
    if E is not None and obs.shape[0] != E:
        raise ValueError(f"per-env obstacles hold one list per env: E = {E}, got {obs.shape[0]} lists")
    if obs.shape[1] > MAX_ENV_OBSTACLES:
        raise ValueError(f"at most {MAX_ENV_OBSTACLES} obstacles per env, got M = {obs.shape[1]}")
    if M is not None and obs.shape[1] != M:
        raise ValueError(f"M is fixed at construction: this field holds {M} rows per env, got {obs.shape[1]}")
    if not np.isfinite(obs).all():
        raise ValueError("obstacles must be finite")
    if (obs[:, :, 2] < 0).any():
        raise ValueError("obstacle radii must be >= 0")
    n_envs, rows = obs.shape[:2]
    if counts is None:
        return obs, np.full(n_envs, rows, np.int64)
    try:
        cnt = np.array(counts)
    except (TypeError, ValueError):
        raise ValueError(f"counts must be [E] integers, got {type(counts).__name__}") from None
    if cnt.shape != (n_envs,) or cnt.dtype == np.bool_ or not np.issubdtype(cnt.dtype, np.integer):
        raise ValueError(f"counts must be [E] = ({n_envs},) integers, got {cnt.dtype} {cnt.shape}")
    if ((cnt < 0) | (cnt > rows)).any():
        raise ValueError(f"counts must be in 0..M = 0..{rows}, got {int(cnt.min())}..{int(cnt.max())}")
    return obs, cnt.astype(np.int64)


def env_obstacle_plan(N, M, m=1):
    """`dronesim_env_obstacle_plan`, a host query: how the per-env kernels reach their lists at ``N`` agents, ``M`` rows per env
    and ``m`` slots -- ``dict(staged=bool, rows_per_block=int, lds_bytes=int)``: staged in LDS per workgroup or read directly, the
    most rows (envs) a 256-record workgroup touches, and the most LDS a workgroup holds.  Needs the library, no GPU."""
    import ctypes as C
    from . import _native
    staged, rows, lds = C.c_int(0), C.c_int(0), C.c_size_t(0)
    _native.call("dronesim_env_obstacle_plan", int(N), int(M), int(m), C.byref(staged), C.byref(rows), C.byref(lds))
    return dict(staged=bool(staged.value), rows_per_block=int(rows.value), lds_bytes=int(lds.value))


def check_m(m):
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= MAX_SENSE:
        raise ValueError(f"m (list slots per agent) must be an integer in 1..{MAX_SENSE}, got {m!r}")
    return int(m)


def check_weight(weight):
    """The obstacle cost's weight as a float: a finite number >= 0 that float32 holds, else ValueError."""
    import numbers
    if isinstance(weight, bool) or not isinstance(weight, numbers.Real) or not 0.0 <= float(weight) <= float(np.finfo(np.float32).max):
        raise ValueError(f"the obstacle weight must be a finite number >= 0, got {weight!r}")
    return float(weight)


def place_obstacles(grid, n, seed=0, keep_clear=None, clearance=0.0, centres=None):
    """Host numpy: ``n`` discs of the reference's sizes (drone_env.py:155-169: radius uniform in ``[0.005, 0.1] max(grid)``) with
    centres uniform in the grid -- or the given ``centres [n,2]`` --, minus the ones that come within ``clearance`` of a point of
    ``keep_clear [P,2]`` (``|centre - point| - r <= clearance``): pass the goals (``env.end_points.reshape(N, 2)``) and e.g. the
    starts -- under the shield a goal inside a disc cannot be reached.  Returns float64 ``[M,3]`` with ``M <= n``; the same ``seed``
    gives the same discs."""
    grid = np.asarray(grid, np.float64).reshape(-1)
    if grid.shape[0] != 2 or not (grid > 0).all():
        raise ValueError(f"grid must be two positive extents, got {grid!r}")
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"n must be an integer >= 0, got {n!r}")
    n = int(n)
    if not 0.0 <= float(clearance) < np.inf:
        raise ValueError(f"clearance must be finite and >= 0, got {clearance!r}")
    rng = np.random.default_rng(seed)
    draw = rng.random((n, 3))
    max_size = 0.1 * grid.max()
    min_size = 0.05 * max_size
    obs = np.empty((n, 3))
    if centres is None:
        obs[:, 0], obs[:, 1] = draw[:, 0] * grid[0], draw[:, 1] * grid[1]
    else:
        centres = np.asarray(centres, np.float64)
        if centres.shape != (n, 2) or not np.isfinite(centres).all():
            raise ValueError(f"centres must be a finite [n,2] = ({n}, 2) array, got shape {centres.shape}")
        obs[:, :2] = centres
    obs[:, 2] = draw[:, 2] * (max_size - min_size) + min_size
    if keep_clear is not None and n:
        pts = np.asarray(keep_clear, np.float64).reshape(-1, 2)
        if not np.isfinite(pts).all():
            raise ValueError("keep_clear must be finite")
        if pts.shape[0]:
            d = np.sqrt(((obs[:, None, :2] - pts[None]) ** 2).sum(2)) - obs[:, None, 2]
            obs = obs[(d > float(clearance)).all(1)]
    return obs


def place_obstacles_per_env(grid, n, E, seed=0, keep_clear=None, clearance=0.0):
    """Host numpy: a list per env.  Env ``e``'s discs are exactly ``place_obstacles(grid, n, seed=[seed, e], keep_clear=...,
    clearance=...)``, zero-padded to ``n`` rows.  Returns ``(obstacles [E,n,3] float64, counts [E] int64)`` -- what
    ``ObstacleField(env, obstacles, per_env=True, counts=counts)`` and ``field.set(obstacles, counts)`` take."""
    if isinstance(E, bool) or int(E) != E or E < 1:
        raise ValueError(f"E must be an integer >= 1, got {E!r}")
    if isinstance(seed, bool) or int(seed) != seed or seed < 0:
        raise ValueError(f"seed must be an integer >= 0, got {seed!r}")
    lists = [place_obstacles(grid, n, seed=[int(seed), e], keep_clear=keep_clear, clearance=clearance) for e in range(int(E))]
    obs = np.zeros((int(E), int(n), 3))
    for e, discs in enumerate(lists):
        obs[e, :discs.shape[0]] = discs
    return obs, np.array([discs.shape[0] for discs in lists], np.int64)


def _obstacle_safety_shapes(z, done, xF, radius, obstacles, z_final, per_env=False):
    """(T, E, N, d) of `episode_obstacle_safety`'s arguments, or ValueError -- shapes, dtypes and devices only."""
    import torch
    if not all(torch.is_tensor(x) for x in (z, done, xF, radius, obstacles)) or z.dim() != 4:
        raise ValueError(f"z must be a [T,E,N,(k+1)c] tensor and done, xF, radius, obstacles tensors, got z {tuple(getattr(z, 'shape', ()))}")
    T, E, N, d = (int(x) for x in z.shape)
    if not 1 <= N <= _MAX_AGENTS or d < 2:
        raise ValueError(f"N must be in 1..{_MAX_AGENTS} and a record hold row 0 (2 floats or more), got N = {N}, {d} floats")
    dev = z.device
    if dev.type != "cuda":
        raise ValueError(f"the obstacle tables work on ROCm device tensors only (no CPU fallback), got z on {dev}")
    _tensor_check("z", z, torch.float32, (T, E, N, d), dev)
    _tensor_check("done", done, torch.uint8, (T, E), dev)
    _tensor_check("xF", xF, torch.float32, (N, 2), dev)
    _tensor_check("radius", radius, torch.float32, (N,), dev)
    if per_env:
        if obstacles.dim() != 3 or tuple(obstacles.shape[::2]) != (E, 3) or obstacles.shape[1] > MAX_ENV_OBSTACLES:
            raise ValueError(f"per-env obstacles must be [E,M,3] = [{E},M,3] with M <= {MAX_ENV_OBSTACLES}, got {tuple(obstacles.shape)}")
    elif obstacles.dim() != 2 or obstacles.shape[1] != 3 or obstacles.shape[0] > MAX_OBSTACLES:
        raise ValueError(f"obstacles must be [M,3] with M <= {MAX_OBSTACLES}, got {tuple(obstacles.shape)}")
    _tensor_check("obstacles", obstacles, torch.float32, tuple(obstacles.shape), dev)
    if z_final is not None:
        _tensor_check("z_final", z_final, torch.float32, (T, E, N, d), dev)
    return T, E, N, d


def episode_obstacle_safety(z, done, xF, radius, obstacles, c, z_final=None, out=None):
    """`dronesim_episode_obstacle_safety` on device tensors: the post-step observations ``z [T,E,N,(k+1)c]`` float32
    (`RolloutStorage.z`), ``done [T,E]`` uint8, the goals ``xF [N,2]``, ``radius [N]`` and the discs ``obstacles [M,3]`` float32,
    ``c`` (2 or 5) floats per row, and the terminal observations ``z_final`` of an auto_reset window.  The obstacle tables of the
    FIRST episode of every env (`evaluate.episode_safety`'s episode, the same ``ep_len``): ``min_obstacle_gap [E,N]`` float32, the
    smallest gap of the agent to any disc over the episode; ``obstacle_hit_steps [E,N]`` int32, the steps at which it touched or
    overlapped one (``gap <= 0``); ``ep_min_obstacle_gap [E]`` float32 and ``ep_obstacle_hit_steps [E]`` int32 over the agents;
    ``ep_len [E]`` int32.  Envs without an episode get NaN and 0; the minimum keeps a NaN; ``M = 0`` gives ``+inf`` and 0.  ``out``: a
    dict of tensors to write into (the entries it lacks are not computed, except ``ep_len``; a per-env table needs the per-agent
    one it reduces)."""
    import torch
    from . import _native
    T, E, N, d = _obstacle_safety_shapes(z, done, xF, radius, obstacles, z_final)
    if c not in (2, 5) or d % c:
        raise ValueError(f"c must be 2 or 5 and divide the record's {d} floats, got {c!r}")
    k1, M = d // c, int(obstacles.shape[0])
    out = _safety_tables(out, E, N, z.device)
    _native.call("dronesim_episode_obstacle_safety", z, z_final, done, xF, radius, obstacles if M else None, T, E, N, k1, c, M,
                 out["ep_len"], out.get("min_obstacle_gap"), out.get("obstacle_hit_steps"), out.get("ep_min_obstacle_gap"),
                 out.get("ep_obstacle_hit_steps"))
    return out


def episode_env_obstacle_safety(z, done, xF, radius, obstacles, counts, c, z_final=None, out=None):
    """`dronesim_episode_env_obstacle_safety`: `episode_obstacle_safety` with a list per env -- ``obstacles [E,M,3]`` float32 and
    ``counts [E]`` int32 on the device (``None``: every env holds ``M`` discs), env ``e`` reading its rows ``0..counts[e]-1`` for the
    whole window.  The same five tables; an env without discs gets ``+inf`` and 0, as ``M = 0`` does there."""
    import torch
    from . import _native
    T, E, N, d = _obstacle_safety_shapes(z, done, xF, radius, obstacles, z_final, per_env=True)
    if c not in (2, 5) or d % c:
        raise ValueError(f"c must be 2 or 5 and divide the record's {d} floats, got {c!r}")
    if counts is not None:
        _tensor_check("counts", counts, torch.int32, (E,), z.device)
    k1, M = d // c, int(obstacles.shape[1])
    out = _safety_tables(out, E, N, z.device)
    _native.call("dronesim_episode_env_obstacle_safety", z, z_final, done, xF, radius, obstacles if M else None, counts, T, E, N,
                 k1, c, M, out["ep_len"], out.get("min_obstacle_gap"), out.get("obstacle_hit_steps"),
                 out.get("ep_min_obstacle_gap"), out.get("ep_obstacle_hit_steps"))
    return out


def _safety_tables(out, E, N, dev):
    """`episode_obstacle_safety`'s ``out``, checked, or new tables."""
    import torch
    shapes = dict(ep_len=(torch.int32, (E,)), min_obstacle_gap=(torch.float32, (E, N)), obstacle_hit_steps=(torch.int32, (E, N)),
                  ep_min_obstacle_gap=(torch.float32, (E,)), ep_obstacle_hit_steps=(torch.int32, (E,)))
    if out is not None:
        for name, t in out.items():
            if name not in shapes:
                raise ValueError(f"out[{name!r}] is no obstacle table: {tuple(shapes)}")
            _tensor_check(f"out[{name!r}]", t, shapes[name][0], shapes[name][1], dev)
        if "ep_len" not in out:
            raise ValueError("out needs ep_len")
    if out is None:
        out = {name: torch.empty(shape, dtype=dtype, device=dev) for name, (dtype, shape) in shapes.items()}
    return out


class ObstacleField:
    """The static discs of a batched `drones` env, on its device.

        field = ObstacleField(env, place_obstacles(env.grid, 8, seed=1, keep_clear=env.end_points.reshape(-1, 2)), m=2)
        orow, oid = field.sense()                               # [E,N,m,3], [E,N,m] from env.z
        shield = ActionShield(env, 0.25, 0.05, 1.0, obstacles=field)
        tables = field.episode_safety(storage)

    ``obstacles``: ``[M,3]`` (x, y, r), default ``env.obstacles``; ``M`` (0..1024) is fixed at construction, `set` re-uploads other
    discs IN PLACE, so captured graphs see them.  ``env.reset(renew_obstacles=True)`` redraws ``env.obstacles``; the field follows
    only through ``field.set(env.obstacles)``.  ``m``: list slots per agent, 1..4.  ``sense``: the range per agent ``[N]`` (a scalar
    serves all), default the env's Delta (``env.deltas``, read live).  ValueError for a wrong shape, non-finite entries, ``r < 0``,
    ``M > 1024`` or ``m`` outside 1..4 -- before anything touches a device.

    ``sense(z=None, gap_min=False)`` returns ``(orow, oid)`` of the observation ``z`` (default ``env.z``; any observation of the
    env's shape serves: a `RolloutStorage` ring slot, ``z_final``): slot ``s`` of ``orow [E,N,m,3]`` is ``(p.x, p.y, r)`` of the
    ``s``-th nearest disc in range and ``oid [E,N,m]`` its id, empty slots ``(0, 0, 0)`` and -1.  With ``gap_min=True`` the
    attributes ``gap_min [E,N]`` (over ALL discs, ``+inf`` at ``M = 0``) and ``hit [E,N]`` uint8 are written too.  The buffers are
    allocated by the first call (the planes by the first call that asks for them) and reused: after an eager warm-up the calls
    can be captured in a ``torch.cuda.graph``.

    ``per_env=True``: ``obstacles`` is ``[E,M,3]`` with ``E == env.n_envs`` and ``M <= 64``, one list per env, and ``counts [E]``
    integers in ``0..M`` (default all ``M``) say how many rows of each env are discs (`check_env_obstacles`; without ``per_env`` a
    3-D array is still refused).  ``M`` and ``E`` are fixed at construction; ``set(obstacles, counts=None)`` re-uploads discs and
    counts IN PLACE.  `sense`, `observe`, `shape_reward` and `episode_safety` then run the per-env entries, with the same return
    shapes, buffers and reuse; ids in ``oid`` are env-local.  `observe` needs leading dims that end in ``E`` (row ``q`` belongs to
    env ``q % E``).  Attributes: ``per_env``, ``counts`` (int64 ``[E]``, None for a shared list), ``device_obstacles [E,M,3]``."""

    def __init__(self, env, obstacles=None, m=2, sense=None, per_env=False, counts=None):
        if not getattr(env, "batched", False):
            raise ValueError("ObstacleField needs the batched (tensor) API of `drones`")
        self.m = check_m(m)
        self.per_env = bool(per_env)
        if self.per_env:
            if obstacles is None:
                raise ValueError("per_env=True needs obstacles [E,M,3] (the env draws one list)")
            obs, cnt = check_env_obstacles(obstacles, counts, E=int(env.n_envs))
        else:
            if counts is not None:
                raise ValueError("counts needs per_env=True")
            obs, cnt = check_obstacles(env.obstacles if obstacles is None else obstacles), None
        N = int(env.n_agents)
        if sense is not None:
            sense = np.array(sense, np.float64)
            sense = np.full(N, float(sense)) if sense.ndim == 0 else sense
            if sense.shape != (N,) or np.isnan(sense).any():
                raise ValueError(f"sense must be a number or [N] = ({N},) numbers, got shape {sense.shape}")
        import torch
        self.env, self.M = env, int(obs.shape[-2])
        self.obstacles, self.counts = obs, cnt
        if self.per_env:                                       # [E,M,3] and the counts; at M = 0 the entries take NULL lists
            self._obs = self._obs_view = torch.zeros(int(env.n_envs), self.M, 3, dtype=torch.float32, device=env.device)
            self._counts = torch.zeros(int(env.n_envs), dtype=torch.int32, device=env.device)
        else:
            # (at least one row, so that the tensor has an address at M = 0; the kernels read M rows)
            self._obs = torch.zeros(max(self.M, 1), 3, dtype=torch.float32, device=env.device)
            self._obs_view = self._obs[:self.M]
        self._sense = None if sense is None else torch.tensor(sense, dtype=torch.float32, device=env.device)
        self.orow = self.oid = self.gap_min = self.hit = None
        self.cost = None                                       # `observe(cost=...)`'s plane of its last call
        self._x, self._cost = {}, {}                           # `observe`'s owned buffers, per leading shape
        self.set(obs, cnt)

    @property
    def _lists(self):
        """The per-env entries' ``obstacles`` argument: NULL at ``M = 0``."""
        return self._obs if self.M else None

    @property
    def sense_range(self):
        """The range per agent, float32 ``[N]`` on the device (the env's Delta unless the field was given its own)."""
        return self.env._delta if self._sense is None else self._sense

    @property
    def device_obstacles(self):
        """The discs as the kernels read them: float32 ``[M,3]`` (``[E,M,3]`` with ``per_env``) on the env's device."""
        return self._obs_view

    def set(self, obstacles, counts=None):
        """Other discs, the same count ``M`` (and, with ``per_env``, other ``counts``, default all ``M``): re-uploaded into the
        same device memory."""
        import torch
        if self.per_env:
            obs, cnt = check_env_obstacles(obstacles, counts, E=int(self.env.n_envs), M=self.M)
            self.obstacles, self.counts = obs, cnt
            if self.M:
                self._obs.copy_(torch.as_tensor(obs.astype(np.float32)))
            self._counts.copy_(torch.as_tensor(cnt.astype(np.int32)))
            return self
        if counts is not None:
            raise ValueError("counts needs per_env=True")
        obs = check_obstacles(obstacles, self.M)
        self.obstacles = obs
        if self.M:
            self._obs_view.copy_(torch.as_tensor(obs.astype(np.float32)))
        return self

    def sense(self, z=None, gap_min=False):
        import torch
        from . import _native
        env = self.env
        E = int(env.n_envs)
        N, k1, c = self._geometry()
        z = env.z if z is None else z
        dev = torch.device(env.device)
        _tensor_check("z", z, torch.float32, (E, N, k1 * c), dev)
        xF, radius, rng = self._env_tensors(dev)
        if self.orow is None:
            self.orow = torch.zeros(E, N, self.m, 3, dtype=torch.float32, device=dev)
            self.oid = torch.full((E, N, self.m), -1, dtype=torch.int32, device=dev)
        if gap_min and self.gap_min is None:
            self.gap_min = torch.zeros(E, N, dtype=torch.float32, device=dev)
            self.hit = torch.zeros(E, N, dtype=torch.uint8, device=dev)
        planes = (self.gap_min if gap_min else None, self.hit if gap_min else None)
        if self.per_env:
            _native.call("dronesim_env_obstacle_sense", z, xF, radius, rng, self._lists, self._counts, E, N, k1, c, self.M, self.m,
                         self.orow, self.oid, *planes)
        else:
            _native.call("dronesim_obstacle_sense", z, xF, radius, rng, self._obs, E, N, k1, c, self.M, self.m, self.orow, self.oid,
                         *planes)
        return self.orow, self.oid

    @property
    def obs_width(self):
        """Floats per agent of `observe`'s output: the record's ``(k+1)c`` plus three per list slot."""
        return (int(self.env.k_closest) + 1) * int(self.env.c) + 3 * self.m

    def _geometry(self):
        env = self.env
        N, k1, c = int(env.n_agents), int(env.k_closest) + 1, int(env.c)
        if not 1 <= N <= _MAX_AGENTS or not 1 <= k1 <= _MAX_K + 1 or c not in (2, 5):
            raise ValueError(f"the obstacle entries need N in 1..{_MAX_AGENTS}, k + 1 in 1..{_MAX_K + 1} and c in (2, 5), got N = {N}, "
                             f"k + 1 = {k1}, c = {c}")
        return N, k1, c

    def _env_tensors(self, dev):
        import torch
        env, rng = self.env, self.sense_range
        N = int(env.n_agents)
        for name, x, shape in (("xF", env._xF, (N, 2)), ("radius", env._radius, (N,)), ("sense", rng, (N,))):
            _tensor_check(name, x, torch.float32, shape, dev)
        return env._xF, env._radius, rng

    def observe(self, z=None, out=None, cost=None):
        """`dronesim_obstacle_observe`: the networks' input with the obstacle columns.  ``z [..., N, (k+1)c]`` (default ``env.z``;
        the leading dims are rows: a `RolloutStorage` ring ``z_all``, the learner's ``z_trunc``, one step) gives
        ``x [..., N, (k+1)c + 3m]``: the record's own bits, then slot ``s`` of `sense`'s list as ``(p.x, p.y, r)``, ``(0, 0, 0)`` where
        it is empty.  Returns ``out`` (a contiguous float32 tensor of that shape), or an owned buffer that is reused for every later
        input of this shape.  ``cost=weight`` (finite, >= 0) also fills the attribute ``cost [..., N]``, ``weight`` times the
        obstacle cost of every record (include/dronesim.h has the rule).  One launch; capturable after an eager warm-up."""
        import torch
        from . import _native
        N, k1, c = self._geometry()
        d = k1 * c
        z = self.env.z if z is None else z
        weight = 0.0 if cost is None else check_weight(cost)
        dev = torch.device(self.env.device)
        if not torch.is_tensor(z) or z.dim() < 2 or tuple(z.shape[-2:]) != (N, d):
            raise ValueError(f"z must be a [..., N, (k+1)c] = [..., {N}, {d}] tensor, got {tuple(getattr(z, 'shape', ()))}")
        lead = tuple(int(n) for n in z.shape[:-2])
        E = int(self.env.n_envs)
        if self.per_env and (not lead or lead[-1] != E):
            raise ValueError(f"with per-env obstacles the leading dims of z must end in E = {E} (row q belongs to env q % E), got "
                             f"{tuple(z.shape)}")
        _tensor_check("z", z, torch.float32, lead + (N, d), dev)
        if out is not None:
            _tensor_check("out", out, torch.float32, lead + (N, self.obs_width), dev)
        xF, radius, rng = self._env_tensors(dev)
        if out is None:
            out = self._x.get(lead)
            if out is None:
                out = self._x[lead] = torch.empty(lead + (N, self.obs_width), dtype=torch.float32, device=dev)
        cost_out = None
        if cost is not None:
            cost_out = self._cost.get(lead)
            if cost_out is None:
                cost_out = self._cost[lead] = torch.empty(lead + (N,), dtype=torch.float32, device=dev)
            self.cost = cost_out
        R = int(np.prod(lead, dtype=np.int64)) if lead else 1
        if self.per_env:
            _native.call("dronesim_env_obstacle_observe", z, xF, radius, rng, self._lists, self._counts, R, E, N, k1, c, self.M,
                         self.m, out, cost_out, weight)
        else:
            _native.call("dronesim_obstacle_observe", z, xF, radius, rng, self._obs, R, N, k1, c, self.M, self.m, out, cost_out, weight)
        return out

    def shape_reward(self, storage, weight, out=None, cost_out=None):
        """`dronesim_obstacle_reward` on a `RolloutStorage` of this env: ``reward[t] - weight * cost(observation after step t)``, the
        observation being ``storage.z_final[t]`` where ``done[t]`` (auto_reset) and the post-step ring slot otherwise -- the
        substitution of ``storage.next_z()``.  Returns ``out [T,E,N]`` (default: a new tensor; ``out=storage.reward`` shapes in
        place -- ``storage.reward`` is never written otherwise); ``cost_out [T,E,N]`` receives the weighted cost."""
        import torch
        from . import _native
        N, k1, c = self._geometry()
        weight = check_weight(weight)
        env = self.env
        if getattr(storage, "env", None) is not env:
            raise ValueError("storage must be a RolloutStorage of this field's env")
        dev = torch.device(env.device)
        T, E = (int(n) for n in storage.reward.shape[:2])
        _tensor_check("storage.reward", storage.reward, torch.float32, (T, E, N), dev)
        _tensor_check("storage.z", storage.z, torch.float32, (T, E, N, k1 * c), dev)
        _tensor_check("storage.done", storage.done, torch.uint8, (T, E), dev)
        if storage.z_final is not None:
            _tensor_check("storage.z_final", storage.z_final, torch.float32, (T, E, N, k1 * c), dev)
        for name, t in (("out", out), ("cost_out", cost_out)):
            if t is not None:
                _tensor_check(name, t, torch.float32, (T, E, N), dev)
        xF, radius, rng = self._env_tensors(dev)
        if out is None:
            out = torch.empty(T, E, N, dtype=torch.float32, device=dev)
        if self.per_env:
            if E != int(env.n_envs):
                raise ValueError(f"the storage holds {E} envs, the field {int(env.n_envs)} lists")
            _native.call("dronesim_env_obstacle_reward", storage.z, storage.z_final, storage.done, storage.reward, xF, radius, rng,
                         self._lists, self._counts, T, E, N, k1, c, self.M, weight, out, cost_out)
        else:
            _native.call("dronesim_obstacle_reward", storage.z, storage.z_final, storage.done, storage.reward, xF, radius, rng,
                         self._obs, T, E, N, k1, c, self.M, weight, out, cost_out)
        return out

    def episode_safety(self, storage, out=None):
        """The obstacle tables of a `RolloutStorage` window of this env (`episode_obstacle_safety`): from its stored post-step
        observations (the terminal ones under auto_reset), the env's goals and live radii, and this field's discs."""
        env = self.env
        if getattr(storage, "env", None) is not env:
            raise ValueError("storage must be a RolloutStorage of this field's env")
        if self.per_env:
            return episode_env_obstacle_safety(storage.z, storage.done, env._xF, env._radius, self._obs, self._counts, int(env.c),
                                               storage.z_final, out=out)
        return episode_obstacle_safety(storage.z, storage.done, env._xF, env._radius, self._obs_view, int(env.c), storage.z_final, out=out)
