"""Per-agent learner step of the batched networks (SAC_agents.py:280-357, `SA2CAgents.train_NN`).

The reference trains its N actors and N critics one by one in Python, with torch autograd, once per episode.  Here the
N networks of a `BatchedMLP` are trained together by the HIP library (csrc/learner.hip, exact float32):

  mlp_gradients   dronesim_mlp_grad    per-agent loss gradients over all rows of a window, in one flat buffer
  BatchedAdam     dronesim_adam_step   clip_grad_norm_(max_norm) + torch.optim.Adam, per agent, in place on the weights
  SA2CLearner                          critic update, baseline from the post-update critic, actor update (train_NN)
  PPOLearner      dronesim_mlp_logp, dronesim_neighbour_advantage, dronesim_mlp_grad_ppo
                                       `SPPOAgents.train` (SAC_agents.py:410-573): clipped probability ratio, `epochs`
                                       critic-and-actor steps per window
  lam= of both    dronesim_lambda_returns   bootstrapped lambda-returns (TD(lambda) / GAE) from the critic over the storage's
                                       T+1-slot observation ring, for windows that cut episodes (default off)
  time_limit= of both  dronesim_episode_ends, dronesim_lambda_returns_ends   with ``"bootstrap"`` a time-limit episode end is a
                                       truncation: its return bootstraps from the critic's value of the episode's terminal
                                       observation (``storage.z_final``) instead of stopping there (default ``"terminal"``)
  ent_coef= of both    dronesim_mlp_grad_ent, dronesim_mlp_grad_ppo_ent   an entropy bonus in the actor loss, -ent_coef x the
                                       mean row entropy of the window (default 0: off, the calls above)
  normalize_advantage= of PPOLearner   dronesim_standardize   agent i's advantages standardised over the window's T E rows,
                                       once per window before the epochs (default off)
  target_kl= of PPOLearner             dronesim_mlp_grad_ppo_gated, dronesim_kl_gate, dronesim_adam_step_gated   per-agent KL early
                                       stop decided and obeyed on the device: an actor whose non-negative KL estimate to the
                                       window's old policy passes the threshold takes no further step on this window and costs no
                                       matrix work in the remaining ones; the critic is never gated (default None: off)
  vf_clip= of PPOLearner               dronesim_mlp_grad_vclip   PPO's clipped value loss against the pre-update values of the
                                       window (default None: off)
  minibatches= of PPOLearner           dronesim_row_permutation, dronesim_gather_rows   every epoch reshuffles the window's rows
                                       on the device (a permutation keyed by ``shuffle_seed`` and the critic's device-resident
                                       step counter), gathers them into minibatch-ordered buffers with one launch and takes one
                                       critic and one actor step per minibatch (default 1: off, the whole-window epochs above)

  obs_norm= of both    dronesim_obsnorm_apply, dronesim_obsnorm_update   an `ObsNormalizer`: everything a network reads is
                                       normalised first, with the table as it stands, into learner-owned buffers; the window's
                                       T E pre-step rows are merged into the statistics as ``train()``'s last work (default None)
  reward_norm= of both dronesim_rewnorm_update, dronesim_rewnorm_apply   a `RewardNormalizer` (reward_norm.py): the window is merged
                                       into the running discounted-return statistics, then the return scans read the rewards
                                       times ``1 / std(return)`` from a learner-owned buffer (default None)
  obstacles= of both   dronesim_obstacle_observe, dronesim_obstacle_reward   an `ObstacleField` (obstacles.py): everything a network
                                       reads is first given the field's obstacle columns (the networks' ``d_in`` is
                                       ``field.obs_width``), ahead of ``obs_norm``, and ``obstacle_weight`` times the obstacle cost
                                       of the observation after every step is taken off its reward, ahead of ``reward_norm``, both
                                       into learner-owned buffers; ``train()`` also returns ``obstacle_cost [N]`` (default None)
  share= of BatchedAdam and both   dronesim_adam_step_shared, dronesim_kl_gate_shared, dronesim_mlp_tie   parameter sharing: a
                                       sharing map (`agent_groups`: None, ``"all"`` or a group id per agent) ties the networks of
                                       a group -- one set of weights, the gradient the mean of the members' per-agent gradients,
                                       one Adam state and one norm per group, the PPO gate decided on the group's mean KL;
                                       `BatchedMLP.tie_weights` / `BatchedMLP.take` tie and re-lay-out networks (default None: off)

Flat gradient layout (and Adam's moments): one buffer per network, the six tensors ``w1 | b1 | w2 | b2 | w3 | b3`` each
``[N, ...]`` like `BatchedMLP`'s weights (`flat_layout`).  The learner reads and writes the plain weight arrays
``BatchedMLP.w1 .. b3``; after an update `BatchedAdam.step` re-packs the forward images (`refresh_weights`).

Note on the reference: ``train_NN(buffers, actor_lr)`` only stores ``actor_lr`` in an attribute that nothing reads; the
actors' Adam keeps the lr they were built with (utils.py: ``optim.Adam(self.parameters(), lr=lr)``).  `SA2CLearner` takes
the actor's lr explicitly (``lr_actor``) instead.

Importing this module needs neither a GPU nor the built library; running it needs both (no CPU fallback)."""
from __future__ import annotations

import ctypes as C
import math

TENSOR_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def tensor_shapes(d_in, h1, h2, nout):
    """Per-agent shapes of the six tensors, in flat-buffer order."""
    return ((d_in, h1), (h1,), (h1, h2), (h2,), (h2, nout), (nout,))


def flat_layout(n_agents, d_in, h1, h2, nout):
    """``[(name, offset, shape), ...]`` of the six ``[N, ...]`` tensors in the flat buffer, and its total length."""
    out, off = [], 0
    for name, shp in zip(TENSOR_NAMES, tensor_shapes(d_in, h1, h2, nout)):
        shape = (n_agents,) + shp
        out.append((name, off, shape))
        off += math.prod(shape)
    return out, off


def unflatten(flat, n_agents, d_in, h1, h2, nout):
    """Views ``{name: tensor [N, ...]}`` of a flat gradient / moment buffer."""
    layout, total = flat_layout(n_agents, d_in, h1, h2, nout)
    if flat.numel() != total:
        raise ValueError(f"flat buffer has {flat.numel()} elements, the layout {total}")
    return {name: flat[off:off + math.prod(shape)].view(shape) for name, off, shape in layout}


def action_index(act, n_actions):
    """Index of the entry of the action list (unit vectors at angles ``2 pi a / n``, utils.py:258-265) nearest to each
    stored action ``act [..., 2]`` -- what `log_p_of_a` looks up (utils.py:311-318); the kernel's head does the same."""
    import torch
    ang = torch.atan2(act[..., 1].double(), act[..., 0].double())
    return torch.remainder(torch.round(ang * n_actions / (2 * math.pi)).long(), n_actions)


def plain_struct(mlp):
    """The `DroneMlp` of the learner entry points: the PLAIN weight arrays of `mlp` (``w2_layout = 0``), whatever
    forward image (precision / packing) `mlp` itself evaluates with."""
    from . import _native
    m = _native.DroneMlp()
    m.N, m.d_in, m.h1, m.h2, m.nout = mlp.n_agents, mlp.d_in, mlp.h1, mlp.h2, mlp.nout
    m.out_kind, m.sample_kind, m.w2_layout = mlp.out_kind, 0, 0
    m.w1, m.b1, m.w2 = mlp.w1.data_ptr(), mlp.b1.data_ptr(), mlp.w2.data_ptr()
    m.b2, m.w3, m.b3 = mlp.b2.data_ptr(), mlp.w3.data_ptr(), mlp.b3.data_ptr()
    return m


def grad_workspace_bytes(mlp, rows_per_chunk):
    """Bytes of device workspace `dronesim_mlp_grad` needs at ``rows_per_chunk`` rows per chunk."""
    from . import _native
    return _native.workspace("dronesim_mlp_grad_workspace", C.byref(plain_struct(mlp)), int(rows_per_chunk))


WORKSPACE_BUDGET = 1 << 30          # bytes of gradient workspace per network that the default chunk size aims for


def default_rows_per_chunk(rows, mlp=None, cap=8192, budget=WORKSPACE_BUDGET):
    """Rows per chunk: all rows up to `cap`, a multiple of 64, and -- given the network -- no more than keeps the workspace
    (4 N Rc (h1 + h2 + nout + 1) bytes) within `budget` (at least 64 rows)."""
    rc = min(cap, (rows + 63) // 64 * 64)
    if mlp is not None:
        per_row = 4 * mlp.n_agents * (mlp.h1 + mlp.h2 + mlp.nout + 1)
        rc = min(rc, budget // per_row // 64 * 64)
    return max(64, rc)


class GradientRunner:
    """`dronesim_mlp_grad` and its forms for one network with its own persistent buffers: a call allocates nothing after the
    first of its form."""

    # the forms with a per-agent result beside the loss, by entry point `dronesim_mlp_<form>`: the attribute that keeps the
    # form's workspace bytes, the attribute of the lazily made result tensor, its name in messages and its leading shape
    _FORMS = {"grad_ppo": ("ppo_ws_bytes", "stats", "stats", (4,)),                  # actors: the head's per-row diagnostics
              "grad_ent": ("ent_ws_bytes", "entropy", "entropy", ()),                # actors: + the plane of the row entropies
              "grad_ppo_ent": ("ppo_ent_ws_bytes", "stats5", "stats", (5,)),
              "grad_ppo_gated": ("gated_ws_bytes", "stats6", "stats", (6,)),         # + the k plane and its running sums
              "grad_vclip": ("vclip_ws_bytes", "clip_fraction", "clip_fraction", ())}    # critics: + the zero-gradient flags

    def __init__(self, mlp, rows, rows_per_chunk=None):
        import torch
        self.mlp, self.rows = mlp, int(rows)
        self.rc = int(rows_per_chunk or default_rows_per_chunk(self.rows, mlp))
        self._m = plain_struct(mlp)
        _, total = flat_layout(mlp.n_agents, mlp.d_in, mlp.h1, mlp.h2, mlp.nout)
        self.grad = torch.zeros(total, device=mlp.device)
        self.loss = torch.zeros(mlp.n_agents, device=mlp.device)
        self.ws_bytes = grad_workspace_bytes(mlp, self.rc)
        self.ws = torch.empty(self.ws_bytes // 4, device=mlp.device)

    def _check(self, x, **per_row):
        import torch
        mlp = self.mlp
        if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != self.rows * mlp.n_agents * mlp.d_in:
            raise ValueError(f"x must be a contiguous float32 tensor of {self.rows} rows x {mlp.n_agents} agents x {mlp.d_in}")
        for name, (t, k) in per_row.items():
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.rows * mlp.n_agents * k):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {self.rows} x {mlp.n_agents} x {k}")

    def _workspace(self, form):
        """The workspace bytes and the result tensor of one of `_FORMS`; the first call per form asks the library, grows the one
        shared workspace where this form needs more, and makes the tensor."""
        import torch
        from . import _native
        bytes_attr, out_attr, _, lead = self._FORMS[form]
        if not hasattr(self, out_attr):
            n = _native.workspace(f"dronesim_mlp_{form}_workspace", C.byref(self._m), self.rc)
            if n > self.ws.numel() * 4:
                self.ws = torch.empty((n + 3) // 4, device=self.mlp.device)
            setattr(self, bytes_attr, n)
            setattr(self, out_attr, torch.zeros(*lead, self.mlp.n_agents, device=self.mlp.device))
        return getattr(self, bytes_attr), getattr(self, out_attr)

    def _call(self, form, x, row_scale, head, loss_out=None, out=None):
        """The one call path: ``dronesim_mlp_<form>(m, x, rows, row_scale, *head, grad, loss[, result], chunk, workspace, stream)``
        -- ``head`` are the form's own arguments (tensors, None or numbers) in the entry point's order; ``logp`` has neither
        ``row_scale`` nor gradient and loss.  ``loss_out`` / ``out`` replace ``self.loss`` / the form's own result tensor.
        Returns ``(grad, loss[, result])``."""
        import torch
        from . import _native
        loss = self.loss if loss_out is None else loss_out
        ws_bytes, results = self.ws_bytes, () if form == "logp" else (self.grad, loss)
        if form in self._FORMS:
            ws_bytes, own = self._workspace(form)
            out = own if out is None else out
            if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != own.numel():
                raise ValueError(f"{self._FORMS[form][2]} must be a contiguous float32 tensor {list(own.shape)}")
            results += (out,)
        scale = () if form == "logp" else (float(row_scale),)
        _native.call("dronesim_mlp_" + form, C.byref(self._m), x, self.rows, *scale, *head, *results, self.rc, self.ws, ws_bytes,
                     device=self.mlp.device)
        return (self.grad, loss) if out is None else (self.grad, loss, out)

    def run(self, x, row_scale, target=None, act=None, weight=None, loss_out=None):
        """``loss_out``: a float32 ``[N]`` device tensor that receives the losses instead of ``self.loss``."""
        self._check(x, target=(target, 1), act=(act, 2), weight=(weight, 1))
        return self._call("grad", x, row_scale, (target, act, weight), loss_out)

    def logp(self, x, act, out):
        """`dronesim_mlp_logp`: ``out [rows, N]`` (float32, overwritten) = log pi_i(act | x) under the current weights."""
        self._check(x, act=(act, 2), logp=(out, 1))
        self._call("logp", x, None, (act, out))
        return out

    def run_ppo(self, x, row_scale, act, logp_old, adv, clip_eps, loss_out=None, stats_out=None):
        """`dronesim_mlp_grad_ppo`: returns ``(grad, loss [N], stats [4, N])`` -- stats rows: clipped share, mean
        ``logp_old - logp``, min and max ratio."""
        self._check(x, act=(act, 2), logp_old=(logp_old, 1), adv=(adv, 1))
        return self._call("grad_ppo", x, row_scale, (act, logp_old, adv, float(clip_eps)), loss_out, stats_out)

    def run_ent(self, x, row_scale, act, weight, ent_scale, loss_out=None, entropy_out=None):
        """`dronesim_mlp_grad_ent`: returns ``(grad, loss [N], entropy [N])`` -- the loss is the whole objective
        (``run``'s minus ``ent_scale`` x the summed row entropies), entropy the mean row entropy per agent."""
        self._check(x, act=(act, 2), weight=(weight, 1))
        return self._call("grad_ent", x, row_scale, (act, weight, float(ent_scale)), loss_out, entropy_out)

    def run_ppo_ent(self, x, row_scale, act, logp_old, adv, clip_eps, ent_scale, loss_out=None, stats_out=None):
        """`dronesim_mlp_grad_ppo_ent`: returns ``(grad, loss [N], stats [5, N])`` -- ``run_ppo``'s four rows and the mean row
        entropy; the loss is the whole objective."""
        self._check(x, act=(act, 2), logp_old=(logp_old, 1), adv=(adv, 1))
        return self._call("grad_ppo_ent", x, row_scale, (act, logp_old, adv, float(clip_eps), float(ent_scale)), loss_out, stats_out)

    def run_ppo_gated(self, x, row_scale, act, logp_old, adv, clip_eps, ent_scale, active=None, loss_out=None, stats_out=None):
        """`dronesim_mlp_grad_ppo_gated`: returns ``(grad, loss [N], stats [6, N])`` -- ``run_ppo_ent``'s five rows and the
        non-negative KL estimate (mean of ``expm1(dl) - dl``).  ``active``: int32 ``[N]`` on the device or None; an agent with
        ``active[i] == 0`` is skipped (its gradient slice untouched, its loss and stats NaN)."""
        import torch
        mlp = self.mlp
        self._check(x, act=(act, 2), logp_old=(logp_old, 1), adv=(adv, 1))
        if active is not None and (active.dtype != torch.int32 or not active.is_contiguous() or active.numel() != mlp.n_agents
                                   or active.device != self.grad.device):
            raise ValueError(f"active must be a contiguous int32 tensor [{mlp.n_agents}] on {self.grad.device}")
        return self._call("grad_ppo_gated", x, row_scale, (act, logp_old, adv, float(clip_eps), float(ent_scale), active), loss_out,
                          stats_out)

    def run_vclip(self, x, row_scale, target, v_old, vf_clip, loss_out=None, clip_out=None):
        """`dronesim_mlp_grad_vclip`: returns ``(grad, loss [N], clip_fraction [N])`` -- the loss is the clipped objective
        ``row_scale sum max((V - G)^2, (Vc - G)^2)``, clip_fraction the share of rows whose gradient is zero."""
        self._check(x, target=(target, 1), v_old=(v_old, 1))
        return self._call("grad_vclip", x, row_scale, (target, v_old, float(vf_clip)), loss_out, clip_out)


def mlp_gradients(mlp, x, target=None, act=None, weight=None, row_scale=None, rows_per_chunk=None):
    """Per-agent gradients of `mlp`'s loss over the rows of ``x [..., N, d_in]`` (e.g. ``storage.z_pre [T,E,N,d_in]``):

      critic (out_kind 0):    L_i = row_scale * sum_r (V_i(x_r) - target_r,i)^2               default row_scale 1 / rows (MSE)
      softmax (out_kind 1):   L_i = -row_scale * sum_r weight_r,i log pi_i(a_r,i | x_r)       a from the unit actions ``act``
      Gaussian (out_kind 2):  the same with the Gaussian log density of ``act``                  default row_scale 1 / E

    ``target`` / ``weight`` ``[..., N]``, ``act`` ``[..., N, 2]`` with the leading shape of ``x``; E = ``x.shape[1]`` for a
    4-D ``x`` ([T,E,N,d_in]), 1 otherwise.  Returns ``(grad, loss)``: the flat gradient (`unflatten` gives the tensors)
    and the per-agent losses ``[N]``."""
    import torch
    f = lambda t: None if t is None else t.to(device=mlp.device, dtype=torch.float32).contiguous()
    x = f(x)
    rows = x.numel() // (mlp.n_agents * mlp.d_in)
    if row_scale is None:
        row_scale = 1.0 / rows if mlp.out_kind == 0 else 1.0 / (x.shape[1] if x.dim() == 4 else 1)
    runner = GradientRunner(mlp, rows, rows_per_chunk)
    g, l = runner.run(x, row_scale, f(target), f(act), f(weight))
    return g, l


def agent_groups(share, n_agents):
    """The sharing map ``share`` of ``n_agents`` agents, normalised: ``(group_of, group_ptr, members)``, three lists of ints.

      ``share``      None (nobody shares: N singletons), ``"all"`` (one group) or a length-N sequence of non-negative ints, agent
                     i's group id.  The ids are labels: they need not be contiguous (`evaluate.network_index`'s output is a map).
      ``group_of``   ``[N]``: agent i's group, numbered 0 .. n_groups-1 in the order of the groups' LEADERS, a group's
                     lowest-numbered member.
      ``group_ptr``, ``members``   the same in CSR form (``[n_groups + 1]``, ``[N]``), what the ``dronesim_*_shared`` entry points
                     read: group g's members are ``members[group_ptr[g]:group_ptr[g + 1]]``, ascending, leader first.

    Anything else (another string, a wrong length, a negative, non-integer or bool id) raises ValueError."""
    import numbers
    n = int(n_agents)
    if n < 1:
        raise ValueError(f"n_agents must be >= 1, got {n_agents!r}")
    if share is None:
        ids = list(range(n))
    elif isinstance(share, str):
        if share != "all":
            raise ValueError(f'share must be None, "all" or a sequence of {n} group ids, got {share!r}')
        ids = [0] * n
    else:
        try:
            ids = list(share)
        except TypeError:
            raise ValueError(f'share must be None, "all" or a sequence of {n} group ids, got {share!r}') from None
        if len(ids) != n:
            raise ValueError(f"share has {len(ids)} entries, the network {n} agents")
        for v in ids:
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0:
                raise ValueError(f"share must hold non-negative integers, got {v!r}")
        ids = [int(v) for v in ids]
    number, groups = {}, []
    for i, v in enumerate(ids):                  # agents ascending: a group is first met at its leader
        if v not in number:
            number[v] = len(groups)
            groups.append([])
        groups[number[v]].append(i)
    group_ptr = [0]
    for g in groups:
        group_ptr.append(group_ptr[-1] + len(g))
    return [number[v] for v in ids], group_ptr, [i for g in groups for i in g]


class SharingMap:
    """`agent_groups` of ``share`` uploaded once: ``group_ptr`` / ``members`` as int32 device tensors, ``leader_of`` (a long
    ``[N]`` device tensor, each agent's leader) and ``n_groups``."""

    def __init__(self, share, n_agents, device):
        import torch
        self.group_of, ptr, members = agent_groups(share, n_agents)
        self.n_groups = len(ptr) - 1
        self.group_ptr = torch.tensor(ptr, dtype=torch.int32, device=device)
        self.members = torch.tensor(members, dtype=torch.int32, device=device)
        self.leader_of = torch.tensor([members[ptr[g]] for g in self.group_of], dtype=torch.long, device=device)

    def tied(self, mlp):
        """Whether every member's six plain tensors equal its leader's (synchronises the host)."""
        import torch
        return all(torch.equal(w, w[self.leader_of]) for w in (getattr(mlp, name) for name in TENSOR_NAMES))


class BatchedAdam:
    """clip_grad_norm_(max_norm) + torch.optim.Adam (torch defaults: no weight decay, no amsgrad) for the N networks of
    one `BatchedMLP`, one optimiser state per agent: flat moments ``m1`` / ``m2`` and a per-agent step counter in device
    memory (a captured graph advances it on every replay).  ``step(grad)`` returns the pre-clip norms ``[N]``.
    ``step(grad, active=a)`` (int32 ``[N]`` on the device) is `dronesim_adam_step_gated`: an agent with ``a[i] == 0`` keeps its
    weights, moments, counter and gradient slice, and its norm is NaN.

    ``share`` (default None: exactly the calls above, nothing more allocated) is a sharing map (`agent_groups`), fixed for the
    life of the object: the members of a group hold ONE network.  The CSR arrays are uploaded once, and every member's six
    tensors must already equal its leader's (checked here with ``torch.equal``; `BatchedMLP.tie_weights` makes them so).
    ``step`` is then `dronesim_adam_step_shared`, gated or not: the group's gradient is the mean of its members' slices
    (float64, into the leader's slice), one norm, clip and Adam step on the leader -- its slices of ``m1`` / ``m2`` / ``grad``
    are the only live ones --, then the leader's weights and counter are copied to the members and the group's norm to every
    member's slot.  A gated group's flag is its leader's."""

    def __init__(self, mlp, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=10.0, share=None):
        import torch
        self.mlp = mlp
        self.lr, self.betas, self.eps, self.max_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(max_norm)
        _, total = flat_layout(mlp.n_agents, mlp.d_in, mlp.h1, mlp.h2, mlp.nout)
        self.numel = total
        self.share = None if share is None else SharingMap(share, mlp.n_agents, mlp.device)
        if self.share is not None and not self.share.tied(mlp):
            raise ValueError("share: a member's weights differ from its leader's; call mlp.tie_weights(share) first")
        self.m1 = torch.zeros(total, device=mlp.device)
        self.m2 = torch.zeros(total, device=mlp.device)
        self.steps = torch.zeros(mlp.n_agents, dtype=torch.int32, device=mlp.device)
        self.grad_norm = torch.zeros(mlp.n_agents, device=mlp.device)
        self._m = plain_struct(mlp)

    def step(self, grad, norm_out=None, refresh=True, active=None):
        """``norm_out``: a float32 ``[N]`` device tensor that receives the norms instead of ``self.grad_norm``;
        ``refresh=False`` leaves the network's forward images stale (the caller refreshes them before the next forward);
        ``active``: the per-agent gate of `dronesim_adam_step_gated` (None: `dronesim_adam_step`)."""
        import torch
        from . import _native
        norm = self.grad_norm if norm_out is None else norm_out
        if grad.dtype != torch.float32 or not grad.is_contiguous() or grad.numel() != self.numel or grad.device != self.m1.device:
            raise ValueError(f"grad must be the flat float32 gradient buffer ({self.numel} elements) on {self.m1.device}")
        if active is not None and (active.dtype != torch.int32 or not active.is_contiguous() or active.numel() != self.mlp.n_agents
                                   or active.device != self.m1.device):
            raise ValueError(f"active must be a contiguous int32 tensor [{self.mlp.n_agents}] on {self.m1.device}")
        shared = (C.byref(self._m), grad, self.m1, self.m2, self.steps, self.lr, self.betas[0], self.betas[1], self.eps, self.max_norm, norm)
        if self.share is not None:
            _native.call("dronesim_adam_step_shared", *shared, active, self.share.group_ptr, self.share.members, self.share.n_groups,
                         device=self.mlp.device)
        elif active is None:
            _native.call("dronesim_adam_step", *shared, device=self.mlp.device)
        else:
            _native.call("dronesim_adam_step_gated", *shared, active, device=self.mlp.device)
        if refresh:
            self.mlp.refresh_weights()
        return norm


def _check_lam(lam):
    """``lam=None`` (Monte-Carlo returns inside the window, the reference's rule) or a number in [0, 1]."""
    if lam is None:
        return None
    from .rollout_buffer import check_lam
    return check_lam(lam)


def _check_ent_coef(ent_coef):
    """``ent_coef`` as a finite float >= 0, else ValueError."""
    import numbers
    if isinstance(ent_coef, bool) or not isinstance(ent_coef, numbers.Real) or not math.isfinite(ent_coef) or ent_coef < 0:
        raise ValueError(f"ent_coef must be a finite number >= 0, got {ent_coef!r}")
    return float(ent_coef)


def _check_positive(name, value):
    """None (off) or a finite float > 0, else ValueError."""
    import numbers
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) or value <= 0:
        raise ValueError(f"{name} must be None or a finite number > 0, got {value!r}")
    return float(value)


def _ring(storage, T):
    """The T+1-slot observation ring the bootstrapped returns need (`RolloutStorage.z_all`)."""
    ring = getattr(storage, "z_all", None)
    if ring is None:
        raise ValueError("lam needs the storage's observation ring `z_all` [T+1,E,N,d] (RolloutStorage.z_all: z_pre plus the "
                         "observation after the window's last step); this storage has none")
    if ring.shape[0] != T + 1 or tuple(ring.shape[1:]) != tuple(storage.z_pre.shape[1:]) or not ring.is_contiguous():
        raise ValueError(f"storage.z_all must be a contiguous [T+1,E,N,d] = {(T + 1,) + tuple(storage.z_pre.shape[1:])} tensor, "
                         f"got {tuple(ring.shape)}")
    return ring


def _lambda_returns(learner, storage, Vall, G, reward):
    """`dronesim_lambda_returns` of ``reward`` (the stored rewards, or their normalised image) with the values of all T+1 ring
    slots, into ``G``."""
    from . import _native
    T, E, N = learner._shape
    _native.call("dronesim_lambda_returns", reward, storage.done, Vall, learner.gamma, learner.lam, G, None, T, E, N,
                 device=learner.critic.device)


TIME_LIMITS = ("terminal", "bootstrap")


def _check_time_limit(time_limit, lam):
    """``"terminal"`` or ``"bootstrap"``; the latter needs the critic in the returns, i.e. a ``lam``."""
    if not isinstance(time_limit, str) or time_limit not in TIME_LIMITS:
        raise ValueError(f"time_limit must be one of {TIME_LIMITS}, got {time_limit!r}")
    if time_limit == "bootstrap" and lam is None:
        raise ValueError('time_limit="bootstrap" needs bootstrapped lambda-returns: give a lam in [0, 1] (with lam=None the '
                         "returns are the reference's whole-episode rule, which has no critic in it)")
    return time_limit


def _prepare_ends(learner, storage, T, E, N):
    """Check the storage for ``time_limit="bootstrap"`` and make the learner's buffers of that path (first call per shape)."""
    import torch
    from . import drone_env
    zf = getattr(storage, "z_final", None)
    if zf is None:
        raise ValueError('time_limit="bootstrap" needs the terminal observations `z_final` [T,E,N,d] of an env with '
                         "auto_reset=True (RolloutStorage.z_final); this storage has none")
    if tuple(zf.shape) != tuple(storage.z_pre.shape) or not zf.is_contiguous():
        raise ValueError(f"storage.z_final must be a contiguous [T,E,N,d] = {tuple(storage.z_pre.shape)} tensor, got {tuple(zf.shape)}")
    if learner._shape == (T, E, N):
        return
    dev = learner.critic.device
    M = learner.M = -(-T // drone_env.max_time_steps)        # two time-limit ends of one env are max_time_steps slots apart
    learner.ends = torch.empty(T, E, dtype=torch.uint8, device=dev)
    learner.slot_t = torch.empty(M, E, dtype=torch.int32, device=dev)
    learner.n_trunc = torch.empty(E, dtype=torch.int32, device=dev)
    learner.z_trunc = torch.empty(M, E, N, zf.shape[3], device=dev)
    learner.V_trunc = torch.empty(M * E, N, 1, device=dev)


def _lambda_returns_ends(learner, storage, Vall, G, reward):
    """``time_limit="bootstrap"``: the kinds of the window's episode ends and the terminal observations of the truncated ones
    (`dronesim_episode_ends`), the PRE-update critic over those into ``V_trunc``, then `dronesim_lambda_returns_ends` into ``G``."""
    from . import _native, drone_env
    from .rollout_buffer import _episode_ends
    T, E, N = learner._shape
    M = learner.M
    _episode_ends(storage.done, storage.z_final, drone_env.DONE_RADIUS, M, learner.ends, learner.slot_t, learner.n_trunc,
                  learner.z_trunc)
    z_trunc = learner.z_trunc                                # (the kinds were decided on the RAW z_final: geometry)
    if learner.obstacles is not None:
        z_trunc = learner.obstacles.observe(z_trunc, out=learner._xo_trunc)
    if learner.obs_norm is not None:
        z_trunc = learner.obs_norm.norm(z_trunc, out=learner._xn_trunc)
    learner.critic.forward(z_trunc.view(M * E, N, -1), out=learner.V_trunc)
    _native.call("dronesim_lambda_returns_ends", reward, learner.ends, Vall, learner.V_trunc, M, learner.gamma, learner.lam, G, None,
                 T, E, N, device=learner.critic.device)


def _check_obs_norm(obs_norm, actor, critic):
    """None, or an `ObsNormalizer` whose (N, d) is the networks'."""
    if obs_norm is not None:
        obs_norm.check_networks(actor, critic)
    return obs_norm


def _prepare_obs_norm(learner, storage):
    """The learner's buffers for the normalised observations (first call per shape): the window, or with a ``lam`` the whole
    ring, and under ``time_limit="bootstrap"`` the terminal observations of the truncated ends."""
    import torch
    src = storage.z_pre if learner.lam is None else storage.z_all
    dev, d_in = learner.critic.device, learner.critic.d_in   # (the networks' width: the storage's, plus the obstacle columns)
    learner._xn = torch.empty(tuple(src.shape[:-1]) + (d_in,), device=dev)
    if learner.time_limit == "bootstrap":
        learner._xn_trunc = torch.empty(tuple(learner.z_trunc.shape[:-1]) + (d_in,), device=dev)


def _check_obstacle_inputs(obstacles, obstacle_weight, actor):
    """``(field, weight)``: None and 0.0, or an `ObstacleField` whose ``obs_width`` is the networks' ``d_in`` and a finite weight
    >= 0 of the obstacle cost."""
    if obstacles is None:
        if obstacle_weight != 0.0:
            raise ValueError(f"obstacle_weight = {obstacle_weight!r} needs obstacles= (an ObstacleField)")
        return None, 0.0
    from .obstacles import check_weight
    weight = check_weight(obstacle_weight)
    width, N = getattr(obstacles, "obs_width", None), getattr(getattr(obstacles, "env", None), "n_agents", None)
    if width is None or N is None:
        raise ValueError(f"obstacles must be an ObstacleField, got {type(obstacles).__name__}")
    if (actor.n_agents, actor.d_in) != (int(N), int(width)):
        raise ValueError(f"with obstacles= the networks read the record plus the obstacle columns: {int(N)} agents x "
                         f"field.obs_width = {int(width)} inputs, these read {actor.n_agents} x {actor.d_in}")
    return obstacles, weight


def _raw_width(learner):
    """Floats per record of the storage this learner trains on: the networks' ``d_in``, less the obstacle columns."""
    return learner.critic.d_in - (0 if learner.obstacles is None else 3 * learner.obstacles.m)


def _prepare_obstacles(learner, storage, T, E, N):
    """The learner's buffers of ``obstacles=`` (first call per shape): the augmented window, or with a ``lam`` the augmented ring,
    under ``time_limit="bootstrap"`` the augmented truncated ends, the shaped reward, the weighted cost and its mean per agent."""
    import torch
    if getattr(storage, "env", None) is not learner.obstacles.env:
        raise ValueError("with obstacles= the storage must be a RolloutStorage of the field's env")
    dev, d_in = learner.critic.device, learner.critic.d_in
    learner._xo = torch.empty((T if learner.lam is None else T + 1, E, N, d_in), device=dev)
    if learner.time_limit == "bootstrap":
        learner._xo_trunc = torch.empty(tuple(learner.z_trunc.shape[:-1]) + (d_in,), device=dev)
    learner._rs = torch.empty(T, E, N, device=dev)
    learner._oc = torch.empty(T, E, N, device=dev)
    learner.obstacle_cost = torch.empty(N, device=dev)


def _normalised(learner, storage, T):
    """``(x, ring)``: what the networks read of this window -- the storage's own ``z_pre`` / ``z_all`` without ``obstacles`` and
    an ``obs_norm``; else first their images with the obstacle columns, then those under the normaliser's table as it stands
    (``x`` is the ring's first T slots)."""
    if learner.obstacles is None:
        if learner.obs_norm is None:
            return storage.z_pre, (None if learner.lam is None else storage.z_all)
        if learner.lam is None:
            return learner.obs_norm.norm(storage.z_pre, out=learner._xn), None
        ring = learner.obs_norm.norm(storage.z_all, out=learner._xn)
        return ring[:T], ring
    seen = learner.obstacles.observe(storage.z_pre if learner.lam is None else storage.z_all, out=learner._xo)
    if learner.obs_norm is not None:
        seen = learner.obs_norm.norm(seen, out=learner._xn)
    return (seen, None) if learner.lam is None else (seen[:T], seen)


def _obs_norm_rows(learner, storage, T):
    """What the statistics are fed after a call: the window's T E pre-step rows as the normaliser sees them."""
    return storage.z_pre if learner.obstacles is None else learner._xo[:T]


def _check_reward_norm(reward_norm, actor, share):
    """None, or a `RewardNormalizer` for the networks' N whose statistics groups respect the sharing map ``share`` (a
    `SharingMap` or None): the members of a tied group must share one statistics group -- one critic cannot fit two units."""
    if reward_norm is None:
        return None
    reward_norm.check_agents(actor.n_agents)
    if share is not None:
        unit = {}
        for i, g in enumerate(share.group_of):
            if unit.setdefault(g, reward_norm.group_of[i]) != reward_norm.group_of[i]:
                raise ValueError(f"reward_norm puts the tied agents of sharing group {g} into different statistics groups: one "
                                 'network cannot fit two units (use scope="team" or a map that keeps tied agents together)')
    return reward_norm


def _normalised_reward(learner, storage):
    """What the return scans read: ``storage.reward`` itself without a ``reward_norm``; else the window is first merged into the
    running return statistics (unless ``update_reward_norm=False``) and then scaled into the learner's own ``_rn [T,E,N]`` --
    ``storage.reward`` is never written.  With ``obstacles`` the reward both of them see is the shaped one, in the learner's own
    ``_rs [T,E,N]`` (`ObstacleField.shape_reward`); the weighted cost goes to ``_oc`` and its mean per agent to ``obstacle_cost``."""
    reward = storage.reward
    if learner.obstacles is not None:
        import torch
        reward = learner.obstacles.shape_reward(storage, learner.obstacle_weight, out=learner._rs, cost_out=learner._oc)
        torch.mean(learner._oc.view(-1, learner._oc.shape[-1]), dim=0, out=learner.obstacle_cost)
    if learner.reward_norm is None:
        return reward
    if learner.update_reward_norm:
        learner.reward_norm.update(reward, storage.done)
    return learner.reward_norm.norm(reward, out=learner._rn)


MINIBATCH_ALIGN = 256               # every minibatch's block of a gathered buffer starts on this boundary (bytes)


def _check_minibatches(minibatches, shuffle_seed):
    """``minibatches`` as an int >= 1 and ``shuffle_seed`` as an int in [0, 2^64), else ValueError."""
    import numbers
    if isinstance(minibatches, bool) or not isinstance(minibatches, numbers.Integral) or minibatches < 1:
        raise ValueError(f"minibatches must be an integer >= 1, got {minibatches!r}")
    if isinstance(shuffle_seed, bool) or not isinstance(shuffle_seed, numbers.Integral) or not 0 <= shuffle_seed < 2 ** 64:
        raise ValueError(f"shuffle_seed must be an integer in [0, 2^64), got {shuffle_seed!r}")
    return int(minibatches), int(shuffle_seed)


class GatheredRows:
    """The minibatch-ordered copy of one ``[R, ...]`` float32 array: K blocks of M rows in one persistent buffer, every block
    starting on a `MINIBATCH_ALIGN`-byte boundary (``blocks[b]`` is the contiguous ``[M, ...]`` view of block b), so that the
    gradient entry points see the alignment of a fresh allocation whatever M x the row size is."""

    def __init__(self, row_shape, K, M, device):
        import torch
        self.row_bytes = 4 * math.prod(row_shape)
        self.block_bytes = -(-M * self.row_bytes // MINIBATCH_ALIGN) * MINIBATCH_ALIGN
        self.buf = torch.zeros(K * self.block_bytes // 4, device=device)
        if self.buf.is_cuda and self.buf.data_ptr() % MINIBATCH_ALIGN:
            raise RuntimeError(f"the allocator returned a buffer that is not {MINIBATCH_ALIGN}-byte aligned")
        n, stride = M * self.row_bytes // 4, self.block_bytes // 4
        self.blocks = [self.buf[b * stride:b * stride + n].view(M, *row_shape) for b in range(K)]


class SA2CLearner:
    """`SA2CAgents.train_NN` (SAC_agents.py:280-357) over a `RolloutStorage` window of E envs, T steps:

      1. G = storage.returns(gamma); critic loss per agent = mean over the T E rows of (V_i(x) - G)^2;
         clip to ``max_norm``, one Adam step (lr ``lr_critic``)
      2. V from the POST-update critic (as the reference's actor loop reads ``self.criticsNN[i]``);
         w = storage.advantage(V, gamma, G)  (gamma^t / N sum over the neighbours, restarts at ``done``)
      3. actor loss per agent = -(1/E) sum_{t,e} w log pi_i(a | x); clip, one Adam step (lr ``lr_actor``)

    ``train(storage)`` returns a dict of device tensors ``[N]``: critic_loss, actor_loss, critic_grad_norm,
    actor_grad_norm (pre-clip).  It does not synchronise the host, the HIP entry points enqueue kernels only (no memset nodes), and the
    step counters live in device memory, so a rollout window and the update can be captured in one ``torch.cuda.graph``
    whose replays equal the eager sequence.  Allocation: the learner's own buffers are made on the first call for a storage
    shape; after that the learner allocates nothing itself, BUT every update calls `BatchedMLP.refresh_weights`, whose
    re-packing of the forward images (e.g. `pack_f32_rowtile_stream`) makes temporary tensors through torch's caching
    allocator -- served from its cache eagerly, and from the graph's private pool when captured.  So the issue's "allocates
    nothing after the first call" holds for the learner's buffers, not for those packing temporaries.

    ``lam`` chooses the critic target and the G of the advantage:

      ``lam=None``  (default) the steps above, the reference's rule: Monte-Carlo returns of the rewards INSIDE the window.
                    Right when the window holds whole episodes; a window that cuts an episode (auto_reset, or T below the
                    episode length) truncates that episode's returns to the rewards the window happens to hold.
      ``lam=1.0``   Monte-Carlo with a bootstrap at the window's end: G[T-1] = r + gamma V(z after the window).  Not the
                    same as None; the two agree bit for bit on the columns whose window ends with ``done``.
      ``lam<1``     TD(lambda): G[t] = r[t] + gamma ((1 - lam) V(z[t+1]) + lam G[t+1]); 0 is the one-step target.

    With a ``lam`` step 1 becomes: 1a. V of the PRE-update critic over all T+1 slots of the storage's observation ring
    (``storage.z_all``); 1b. G = `dronesim_lambda_returns` of it (an episode end is terminal: nothing is carried across
    ``done``, and the new episode's values do not leak into the old one); 1c. the critic step on target G.  Steps 2 and 3 are
    unchanged (V from the POST-update critic over ``z_pre``, `dronesim_advantage` with this G).  Cost: one more critic
    forward over (T+1) E rows and one scan.

    ``time_limit`` says what a time-limit episode end (t >= 199 with some agent still outside its goal disk) is to the returns:

      ``"terminal"``   (default) an end like any other, the reference's rule: G[t] = r[t] there, which tells the critic that
                       the cost-to-go at step 199 is zero.
      ``"bootstrap"``  a truncation: G[t] = r[t] + gamma V(terminal observation), whatever ``lam`` is.  Needs a ``lam`` and a
                       storage of an ``auto_reset`` env (``z_final``).  Once per window, ahead of 1b: `dronesim_episode_ends`
                       recovers the kind of every end from ``done`` and ``z_final`` (``ends``, ``slot_t``, ``n_trunc``) and
                       gathers the terminal observations of the truncated ones (``z_trunc [M,E,N,d]``, M = ceil(T / 200)); the
                       PRE-update critic over them gives ``V_trunc [M E,N,1]``; 1b becomes `dronesim_lambda_returns_ends`.  An
                       arrival is terminal as before, also on the last allowed step.  Steps 2 and 3 are unchanged: the
                       advantage still restarts at ``done``.

    ``ent_coef`` (default 0: off, exactly the calls above) adds an entropy bonus to step 3: the actor loss becomes
    ``-(1/E) sum w log pi - ent_coef x the mean over the T E rows of H(pi_i(. | x))`` (`dronesim_mlp_grad_ent` with
    ``ent_scale = ent_coef / (T E)``; the likelihood term keeps its 1 / E), ``actor_loss`` is that whole objective and
    ``train()`` also returns ``entropy [N]``, the mean row entropy under the pre-update actor.  There is NO advantage
    standardisation here (`PPOLearner` has it): this learner's weight ``w`` carries gamma^t / N inside `dronesim_advantage`, and
    standardising it would be another change.

    ``obs_norm`` (default None: exactly the calls above, nothing more allocated) is an `ObsNormalizer` for the networks' (N, d).
    ``train()`` then starts by normalising, with the table as it stands, everything a network reads into buffers of its own --
    ``z_pre``, or with a ``lam`` the whole ring ``z_all`` (x is its first T slots), and under ``time_limit="bootstrap"`` the
    gathered ``z_trunc`` (the kinds of the ends are still decided on the RAW ``z_final``: that is geometry) -- and the table is
    not touched until the last step has been enqueued: the rollout that collected the window and every step of the update see
    one map.  Its last enqueued work, unless ``update_obs_norm=False``, is ``obs_norm.update(storage.z_pre)``: the T E pre-step
    rows only, ring slot T is the next window's slot 0.  A normaliser of another shape raises ValueError.

    ``share`` (default None: exactly the calls above, nothing more allocated) is a sharing map (`agent_groups`) applied to BOTH
    the actor and the critic: the agents of a group train ONE network.  Nothing upstream of the optimiser changes -- every agent
    still gets its own gradient from its own rows, and all per-agent outputs keep their shapes and meaning --; both steps become
    `dronesim_adam_step_shared` (`BatchedAdam`): the group's gradient is the mean of its members', i.e. the gradient of one
    network on the members' pooled rows with row scale ``1 / (|G| rows)``, so ``lr`` and ``max_norm`` keep their meaning.  The
    members' weights must be tied beforehand (`BatchedMLP.tie_weights`; ValueError otherwise) and stay bit-identical after every
    update; the two grad-norm outputs carry the group's norm in every member's slot.

    ``reward_norm`` (default None: exactly the calls above, nothing more allocated) is a `RewardNormalizer` for the networks' N.
    ``train()`` then starts with ``reward_norm.update(storage.reward, storage.done)`` (unless ``update_reward_norm=False``) and
    writes ``reward_norm.norm(storage.reward)`` into a buffer of its own, ``_rn [T,E,N]``; that buffer is what `dronesim_returns`,
    `dronesim_lambda_returns` and `dronesim_lambda_returns_ends` read.  UPDATE FIRST, THEN APPLY -- the other way round than
    ``obs_norm``: no acting kernel has to agree with the reward scale, so nothing forbids changing it ahead of the update, and
    a fresh normaliser (scale 1) would otherwise train its first window on raw rewards.  ``storage.reward`` is never written: the
    `Evaluator` and every logged statistic stay in raw units.  The critic's values (and G, and the advantage) are then in
    NORMALISED units.  ``train()`` also returns ``reward_scale [N]`` (float64, the scale this window was trained with).  A
    normaliser for another N raises ValueError, and so does, with ``share``, one whose statistics groups split a tied group
    (``scope="team"`` always fits).

    ``obstacles`` (default None: exactly the calls above, nothing more allocated) is an `ObstacleField` of the storage's env, for
    obstacle-aware training; the networks' ``d_in`` must be ``field.obs_width`` (the record plus ``3 m`` obstacle columns), else
    ValueError.  The order is raw -> obstacles -> normalisers.  ``train()`` first writes ``field.observe`` of ``z_pre`` (with a
    ``lam``: of the ring) into a buffer of its own, ``_xo``, and THAT is what ``obs_norm`` and the networks read; under
    ``time_limit="bootstrap"`` the end kinds are still decided on the RAW ``z_final`` and ``z_trunc`` is augmented (``_xo_trunc``)
    before the normaliser and the critic.  ``field.shape_reward(storage, obstacle_weight)`` goes into ``_rs [T,E,N]`` (the
    weighted cost into ``_oc``) and THAT is what ``reward_norm`` merges and scales and the return scans read; ``storage.reward``
    is never written.  The statistics' update is fed the augmented ``z_pre``.  ``train()`` also returns ``obstacle_cost [N]``, the
    window's mean weighted cost per agent, on the device.  ``obstacle_weight`` (finite, >= 0; 0 leaves the reward's bits) needs
    ``obstacles``."""

    def __init__(self, actor, critic, gamma, lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0, rows_per_chunk=None, lam=None,
                 time_limit="terminal", ent_coef=0.0, obs_norm=None, update_obs_norm=True, share=None, reward_norm=None,
                 update_reward_norm=True, obstacles=None, obstacle_weight=0.0):
        if critic.out_kind != 0 or critic.nout != 1:
            raise ValueError("the critic must be a BatchedMLP with out_kind 0 and one output")
        if actor.out_kind not in (1, 2):
            raise ValueError("the actor must be a softmax (out_kind 1) or Gaussian (out_kind 2) BatchedMLP")
        if (actor.n_agents, actor.d_in) != (critic.n_agents, critic.d_in):
            raise ValueError("actor and critic must have the same agents and inputs")
        self.actor, self.critic, self.gamma, self.lam = actor, critic, float(gamma), _check_lam(lam)
        self.time_limit = _check_time_limit(time_limit, self.lam)
        self.ent_coef = _check_ent_coef(ent_coef)
        self.obs_norm, self.update_obs_norm = _check_obs_norm(obs_norm, actor, critic), bool(update_obs_norm)
        self.rows_per_chunk = rows_per_chunk
        self.actor_opt = BatchedAdam(actor, lr=lr_actor, max_norm=max_norm, share=share)
        self.critic_opt = BatchedAdam(critic, lr=lr_critic, max_norm=max_norm, share=share)
        self.reward_norm = _check_reward_norm(reward_norm, actor, self.critic_opt.share)
        self.update_reward_norm = bool(update_reward_norm)
        self.obstacles, self.obstacle_weight = _check_obstacle_inputs(obstacles, obstacle_weight, actor)
        self._shape = None

    def _prepare(self, storage):
        import torch
        T, E, N = storage.reward.shape
        if self.lam is not None:
            _ring(storage, T)
        if self.time_limit == "bootstrap":
            _prepare_ends(self, storage, T, E, N)
        if self._shape == (T, E, N):
            return
        if N != self.critic.n_agents or storage.z_pre.shape[-1] != _raw_width(self):
            raise ValueError("the storage's agents / observation width do not match the networks")
        if storage.actions is None:
            raise ValueError("the learner needs a storage with actions")
        dev = self.critic.device
        self.G = torch.empty(T, E, N, device=dev)
        self.V = torch.empty(T * E, N, 1, device=dev)
        self.w = torch.empty(T, E, N, device=dev)
        if self.lam is not None:
            self.V_all = torch.empty((T + 1) * E, N, 1, device=dev)      # the pre-update critic over the whole ring
        self._critic_grad = GradientRunner(self.critic, T * E, self.rows_per_chunk)
        self._actor_grad = GradientRunner(self.actor, T * E, self.rows_per_chunk)
        if self.ent_coef > 0:
            self._actor_grad._workspace("grad_ent")
        if self.obstacles is not None:
            _prepare_obstacles(self, storage, T, E, N)
        if self.obs_norm is not None:
            _prepare_obs_norm(self, storage)
        if self.reward_norm is not None:
            self._rn = torch.empty(T, E, N, device=dev)
        self._shape = (T, E, N)

    def train(self, storage):
        from . import _native
        self._prepare(storage)
        T, E, N = self._shape
        x, ring = _normalised(self, storage, T)
        reward = _normalised_reward(self, storage)
        if self.lam is None:
            _native.call("dronesim_returns", reward, storage.done, self.gamma, self.G, T, E, N, device=self.critic.device)
        else:       # bootstrapped lambda-returns from the pre-update critic over all T+1 ring slots
            self.critic.forward(ring.view((T + 1) * E, N, -1), out=self.V_all)
            (_lambda_returns if self.time_limit == "terminal" else _lambda_returns_ends)(self, storage, self.V_all, self.G, reward)
        # critic (SAC_agents.py:304-324)
        cg, closs = self._critic_grad.run(x, 1.0 / (T * E), target=self.G)
        cnorm = self.critic_opt.step(cg)
        # baseline from the post-update critic, advantage weights (:333-351)
        self.critic.forward(x.view(T * E, N, -1), out=self.V)
        nbr = storage.nbr_pre
        _native.call("dronesim_advantage", self.G, self.V, nbr, storage.done, self.gamma, self.w, T, E, N, int(nbr.shape[3]),
                     device=self.critic.device)
        # actor (:327-357)
        if self.ent_coef > 0:
            ag, aloss, ent = self._actor_grad.run_ent(x, 1.0 / E, storage.actions, self.w, self.ent_coef / (T * E))
            anorm = self.actor_opt.step(ag)
            self._update_obs_norm(storage)
            return self._with_scale(dict(critic_loss=closs, actor_loss=aloss, critic_grad_norm=cnorm, actor_grad_norm=anorm, entropy=ent))
        ag, aloss = self._actor_grad.run(x, 1.0 / E, act=storage.actions, weight=self.w)
        anorm = self.actor_opt.step(ag)
        self._update_obs_norm(storage)
        return self._with_scale(dict(critic_loss=closs, actor_loss=aloss, critic_grad_norm=cnorm, actor_grad_norm=anorm))

    def _with_scale(self, out):
        if self.reward_norm is not None:
            out["reward_scale"] = self.reward_norm.scale
        if self.obstacles is not None:
            out["obstacle_cost"] = self.obstacle_cost
        return out

    def _update_obs_norm(self, storage):
        """``train()``'s last enqueued work: the window's T E pre-step rows into the statistics (ring slot T is the next window's
        slot 0 and is counted there)."""
        if self.obs_norm is not None and self.update_obs_norm:
            self.obs_norm.update(_obs_norm_rows(self, storage, self._shape[0]))


class PPOLearner:
    """`SPPOAgents.train` (SAC_agents.py:410-573) -- PPO with the clipped probability ratio -- over a `RolloutStorage` window
    of E envs, T steps, for all N agents' networks at once:

      1. G = storage.returns(gamma)                                                          (:476-481, restarts at ``done``)
      2. once per window, before any update, per row (t, e) and agent i:
           logp_old = log pi_i(a | x) under the current actor           (:494; Gaussian density with VARIANCE sigma, :558-573;
                                                                         for a softmax actor the stored action's index)
           Q = sum_{j in N_i(t)} G[t, e, j]   (:498-501),   V = V_i(x) from the PRE-update critic (:512)
           Adv = Q - V            ``baseline="once"``: ONE V_i against the neighbour SUM, the reference's form (:513);
           Adv = Q - |N_i| V      ``baseline="per_neighbour"`` (as `train_NN` subtracts it, SAC_agents.py:346)
         no gamma^t and no 1 / N factor
      3. ``epochs`` times (:522-555), critic first, then actor, both over all T E rows:
           critic: mean (V_i(x) - G)^2, clip to ``max_norm``, Adam (lr ``lr_critic``)         -- `SA2CLearner`'s critic step
           actor:  r = exp(logp - logp_old),  L_i = -(1 / (T E)) sum_rows min(r Adv, clamp(r, 1 - clip_eps, 1 + clip_eps) Adv),
                   clip to ``max_norm``, Adam (lr ``lr_actor``)

    The reference class is NOT runnable as written; this is the algorithm its lines state with exactly three repairs:
    the two lines :513-514 swapped (``Qjsum`` is read one line before it is assigned); ``Adv`` a constant (the reference keeps
    the critic's autograd graph in it and reuses it in every epoch, a second ``backward`` through it raises); the actors
    built with an ``lr`` (:423 omits `NormalActorNN`'s required argument, utils.py:59).  Its ``probability_of_ai`` does run
    and is what tests/golden/ppo_n5.npz records.

    ``train(storage)`` returns a dict of device tensors ``[epochs, N]``: critic_loss, actor_loss, critic_grad_norm,
    actor_grad_norm (pre-clip), clip_fraction (share of rows on the clipped branch), approx_kl (mean logp_old - logp),
    ratio_min, ratio_max.  In the first epoch logp is computed by the same kernels on the same weights as logp_old, so the
    ratio is exactly 1 there (clip_fraction 0, approx_kl 0).  Same properties as `SA2CLearner`: softmax or Gaussian actors;
    buffers allocated on the first call per storage shape (the returned tensors are among them: a later call overwrites
    them); no host synchronisation; the HIP entry points enqueue kernels only (no memset nodes); step counters in device
    memory -- a rollout window and the update can be captured in one ``torch.cuda.graph`` whose replays equal the eager
    sequence.  The forward images are re-packed (`BatchedMLP.refresh_weights`, with the temporaries noted at `SA2CLearner`)
    once per network per call, after the last epoch: the epochs themselves read the plain weight arrays.

    ``lam`` as for `SA2CLearner`: ``None`` (default) is step 1 as written, Monte-Carlo returns inside the window; a number in
    [0, 1] widens step 2's once-per-window critic forward to all T+1 slots of ``storage.z_all`` and takes
    G = `dronesim_lambda_returns` of it (1.0: Monte-Carlo plus a bootstrap from the value after the window's last step,
    equal to None bit for bit on columns whose window ends with ``done``; below 1: TD(lambda)); the first T E rows of that
    forward are step 2's V.  No extra forward, epochs unchanged.

    ``time_limit`` as for `SA2CLearner`: ``"terminal"`` (default) keeps every episode end terminal, time-limit ends included
    (the reference's rule); ``"bootstrap"`` (needs a ``lam`` and ``storage.z_final``) classifies the window's ends, runs the
    same pre-update critic over the terminal observations of the truncated ones (``z_trunc`` -> ``V_trunc``) and takes
    G = `dronesim_lambda_returns_ends`.  Everything after G is unchanged.

    Two options, both off by default (then ``train()`` issues exactly the calls above and allocates nothing more):

      ``normalize_advantage``  once per window, right after step 2, agent i's advantages are standardised IN PLACE over the
                    window's T E rows: ``adv = (adv - mean_i) / (std_i + adv_eps)`` (`dronesim_standardize`: float64 sums, the
                    population std, deterministic).  Each agent has its own network and optimiser, so the scale is per agent.
                    The pre-normalisation (mean, std) are kept as ``self.adv_stats [2, N]`` and returned as ``adv_mean`` and
                    ``adv_std``.
      ``ent_coef``  the actor loss of every epoch becomes ``L_i - ent_coef x the mean over the T E rows of H(pi_i(. | x))``
                    (`dronesim_mlp_grad_ppo_ent` with ``ent_scale = ent_coef / (T E)``); ``actor_loss`` is that whole objective.

    With either, ``train()`` also returns ``entropy [epochs, N]``: the mean row entropy under the actor each epoch started
    from.  The diagnostic comes from the entropy head, so ``normalize_advantage`` alone (``ent_coef = 0``) also runs the
    epochs through `dronesim_mlp_grad_ppo_ent` (adding exact zeros: the sibling's gradients and loss bit for bit), grows the
    workspace by the row-entropy plane and makes ``_stats`` five rows.  The first epoch's ratio stays exactly 1 with any
    ``ent_coef``: the old log-probabilities come from the same untouched forward-only pass.

    ``minibatches = K`` (default 1: step 3 as written -- exactly the calls above, nothing more allocated) makes step 3 the usual
    PPO loop of shuffled minibatch epochs.  T E must be a multiple of K (ValueError otherwise; no ragged last minibatch);
    M = T E / K.  Steps 1 and 2 are unchanged and run once per window in window order -- ``normalize_advantage`` stays per
    window, not per minibatch.  Then every epoch:

      a. `dronesim_row_permutation` writes a permutation of the T E rows into ``self.perm`` (int32 ``[T E]``; after ``train`` it
         holds the last epoch's).  It is a pure function of (T E, ``shuffle_seed``, the critic optimiser's step counter of agent
         0): that counter is read ON THE DEVICE, is different for every epoch of every call, and advances on graph replay, so
         a captured ``train`` reshuffles on every replay.  No host generator, no sort.
      b. one `dronesim_gather_rows` copies the permuted rows of ``z_pre``, ``actions``, ``logp_old``, ``adv`` and ``G`` into
         five persistent `GatheredRows` buffers (``self._mb``): minibatch b is rows ``perm[b M : (b + 1) M]``.
      c. for b = 0 .. K-1: the critic step on block b, then the actor step on block b -- the same entry points through
         `GradientRunner`s sized for M rows, with ``row_scale = 1 / M`` and ``ent_scale = ent_coef / M``.

    That is ``epochs x K`` Adam steps per network per call; the forward images are still re-packed once per network, after the
    last minibatch of the last epoch.  The returned per-step tensors become ``[epochs, K, N]`` (``adv_mean`` / ``adv_std`` stay
    ``[N]``).  Only the first minibatch of the first epoch sees the weights ``logp_old`` was computed from, and it sees them in
    another row order and chunking than step 2's forward pass: its ratios are 1 to rounding, not bit for bit.  Everything else
    holds as above: both actor kinds, ``lam``, ``time_limit``, ``ent_coef``, ``normalize_advantage``, ``baseline``, no host
    synchronisation, deterministic, capturable with the rollout in one graph.

    Two guards of those repeated steps on one window, both None by default (then nothing above changes and nothing more is
    allocated); each is a finite number > 0, and both compose with every option above:

      ``target_kl``  per-agent KL early stop.  Nothing in step 3 bounds how far ``epochs x K`` steps carry a policy from the one
                    that collected the window: the ratio clip zeroes the gradient of rows already outside 1 +- clip_eps, it does
                    not stop the walk; and ``approx_kl`` (mean logp_old - logp) changes sign while a policy moves away, so it
                    cannot be thresholded.  The loop cannot ``break`` either (no host synchronisation), so the stop is decided
                    and obeyed ON THE DEVICE through ``self.active`` (int32 ``[N]``): `dronesim_kl_gate` with ``reset`` at the
                    start of every ``train()``; then every actor step, whole-window or minibatch, is
                    `dronesim_mlp_grad_ppo_gated` -> `dronesim_kl_gate` on that step's ``kl`` -> `dronesim_adam_step_gated`.
                    ``kl`` is the non-negative estimate mean(expm1(dl) - dl), dl = logp - logp_old (Schulman's (r - 1) - log r);
                    an agent stops when not ``kl <= target_kl`` (NaN stops, equality continues).  The step on which an agent
                    crosses computes its gradient and discards it; every later actor step of the window skips the agent -- no
                    GEMM tile, head row or sum is computed for it.  The gate is per agent because the agents own their networks
                    and optimisers, and ONLY ACTORS are gated: KL says nothing about the critic, and the row permutation is
                    keyed on the critic's step counter, which must keep advancing.  New outputs: ``kl`` ``[epochs(, K), N]``,
                    ``entropy`` (this is the entropy form of the head, as with ``normalize_advantage``) and ``actor_steps``
                    (int32 ``[N]``: the Adam steps each actor took this window).  The NaN convention: every per-step actor output
                    of a skipped step is NaN; in the crossing step they are real except ``actor_grad_norm``, which is NaN.
      ``vf_clip``   PPO's clipped value loss, the critic's counterpart: its steps go through `dronesim_mlp_grad_vclip` with
                    ``v_old = self.V``, step 2's pre-update values (no extra forward): per row
                    ``max((V - G)^2, (clamp(V, v_old +- vf_clip) - G)^2)``, gradient 0 where the clipped term is the strict
                    maximum.  ``critic_loss`` is that objective; new output ``vf_clip_fraction`` ``[epochs(, K), N]``, the share
                    of zero-gradient rows (exactly 0 in the first step).  With ``minibatches > 1`` V is a sixth gathered array.

    ``obs_norm`` / ``update_obs_norm`` as for `SA2CLearner` (default None: nothing above changes): the window (or ring, and
    ``z_trunc``) is normalised once at the start of ``train()`` with the table as it stands, ``logp_old``, every epoch and the
    minibatch gather read that normalised x -- the first epoch's ratio stays exactly 1 -- and the T E pre-step rows are merged
    into the statistics as the call's last enqueued work.

    ``share`` as for `SA2CLearner` (default None: nothing above changes, nothing more allocated): a sharing map for both
    networks, every Adam step `dronesim_adam_step_shared`.  It composes with every option above.  All per-agent outputs keep
    their shapes and meaning (losses, the PPO diagnostics, ``kl``, ``entropy``, ``adv_*`` are each agent's own, from its own
    rows); the two grad-norm outputs carry the group's norm in every member's slot.  ``normalize_advantage`` STAYS PER AGENT:
    each member's advantages are standardised over its own T E rows before the gradients are pooled, so every member
    contributes at the same scale.  With ``target_kl`` the gate is `dronesim_kl_gate_shared`: a group stops when the MEAN of its
    members' ``kl`` (float64) passes the threshold, all its members together -- ``actor_steps`` is equal within a group.  The
    row permutation still reads ``critic_opt.steps[0]``: the counters are mirrored into every member, so it advances.

    ``reward_norm`` / ``update_reward_norm`` as for `SA2CLearner` (default None: nothing above changes, nothing more allocated):
    the window is merged into the running return statistics first, then scaled into the learner's ``_rn``, which step 1's scan
    reads in ``storage.reward``'s place (update first, then apply; ``storage.reward`` is never written).  G, the critic's values,
    the advantages and therefore ``vf_clip`` are then in NORMALISED units.  New output ``reward_scale [N]``.  With ``share`` the
    statistics groups must keep tied agents together (ValueError otherwise).

    ``obstacles`` / ``obstacle_weight`` as for `SA2CLearner` (default None: nothing above changes, nothing more allocated): the
    window (or ring) and the truncated ends get the field's obstacle columns ahead of ``obs_norm``, the reward pays the weighted
    obstacle cost ahead of ``reward_norm``; minibatches gather the augmented rows.  New output ``obstacle_cost [N]``."""

    BASELINES = ("once", "per_neighbour")

    def __init__(self, actor, critic, gamma, epochs=10, clip_eps=0.2, lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0,
                 baseline="once", rows_per_chunk=None, lam=None, time_limit="terminal", ent_coef=0.0, normalize_advantage=False,
                 adv_eps=1e-8, minibatches=1, shuffle_seed=0, target_kl=None, vf_clip=None, obs_norm=None, update_obs_norm=True,
                 share=None, reward_norm=None, update_reward_norm=True, obstacles=None, obstacle_weight=0.0):
        if critic.out_kind != 0 or critic.nout != 1:
            raise ValueError("the critic must be a BatchedMLP with out_kind 0 and one output")
        if actor.out_kind not in (1, 2):
            raise ValueError("the actor must be a softmax (out_kind 1) or Gaussian (out_kind 2) BatchedMLP")
        if (actor.n_agents, actor.d_in) != (critic.n_agents, critic.d_in):
            raise ValueError("actor and critic must have the same agents and inputs")
        if int(epochs) != epochs or epochs < 1:
            raise ValueError("epochs must be an integer >= 1")
        if not 0.0 < float(clip_eps) < 1.0:
            raise ValueError("clip_eps must be in (0, 1)")
        if baseline not in self.BASELINES:
            raise ValueError(f"baseline must be one of {self.BASELINES}")
        self.actor, self.critic, self.gamma, self.lam = actor, critic, float(gamma), _check_lam(lam)
        self.time_limit = _check_time_limit(time_limit, self.lam)
        self.epochs, self.clip_eps, self.baseline = int(epochs), float(clip_eps), baseline
        self.ent_coef, self.normalize_advantage = _check_ent_coef(ent_coef), bool(normalize_advantage)
        if isinstance(adv_eps, bool) or not math.isfinite(adv_eps) or adv_eps < 0:
            raise ValueError(f"adv_eps must be a finite number >= 0, got {adv_eps!r}")
        self.adv_eps = float(adv_eps)
        self.minibatches, self.shuffle_seed = _check_minibatches(minibatches, shuffle_seed)
        self.target_kl, self.vf_clip = _check_positive("target_kl", target_kl), _check_positive("vf_clip", vf_clip)
        self.obs_norm, self.update_obs_norm = _check_obs_norm(obs_norm, actor, critic), bool(update_obs_norm)
        # the entropy form of the head (and its diagnostics); the gated head is that form
        self._ent = self.ent_coef > 0 or self.normalize_advantage or self.target_kl is not None
        self._stat_rows = 6 if self.target_kl is not None else (5 if self._ent else 4)
        self.rows_per_chunk = rows_per_chunk
        self.actor_opt = BatchedAdam(actor, lr=lr_actor, max_norm=max_norm, share=share)
        self.critic_opt = BatchedAdam(critic, lr=lr_critic, max_norm=max_norm, share=share)
        self.reward_norm = _check_reward_norm(reward_norm, actor, self.critic_opt.share)
        self.update_reward_norm = bool(update_reward_norm)
        self.obstacles, self.obstacle_weight = _check_obstacle_inputs(obstacles, obstacle_weight, actor)
        self._shape = None

    def _prepare(self, storage):
        import torch
        if getattr(storage, "actions", None) is None:
            raise ValueError("the learner needs a storage with actions")
        T, E, N = storage.reward.shape
        if self.lam is not None:
            _ring(storage, T)
        if self.time_limit == "bootstrap":
            _prepare_ends(self, storage, T, E, N)
        if self._shape == (T, E, N):
            return
        if N != self.critic.n_agents or storage.z_pre.shape[-1] != _raw_width(self):
            raise ValueError("the storage's agents / observation width do not match the networks")
        K = self.minibatches
        if (T * E) % K:
            raise ValueError(f"minibatches = {K} does not divide the window's T E = {T} x {E} = {T * E} rows")
        dev = self.critic.device
        self.G = torch.empty(T, E, N, device=dev)
        if self.lam is None:
            self.V = torch.empty(T * E, N, 1, device=dev)
        else:                                                            # the critic over the whole ring; V = its first T E rows
            self.V_all = torch.empty((T + 1) * E, N, 1, device=dev)
            self.V = self.V_all[:T * E]
        self.adv = torch.empty(T, E, N, device=dev)
        self.logp_old = torch.empty(T, E, N, device=dev)
        if K == 1:
            self._critic_grad = GradientRunner(self.critic, T * E, self.rows_per_chunk)
            self._actor_grad = GradientRunner(self.actor, T * E, self.rows_per_chunk)
            self._prepare_forms(self._critic_grad, self._actor_grad)
            self._scalars = torch.zeros(4, self.epochs, N, device=dev)   # critic_loss, actor_loss, critic / actor grad norm
            self._stats = torch.zeros(self.epochs, self._stat_rows, N, device=dev)
            if self.vf_clip is not None:
                self._vclip = torch.zeros(self.epochs, N, device=dev)
        else:
            # the full-window actor runner is kept ONLY for step 2's forward-only `logp` pass, which needs the plain gradient
            # workspace and neither the PPO nor the entropy one (the epochs run through `_critic_mb` / `_actor_mb`)
            self._actor_grad = GradientRunner(self.actor, T * E, self.rows_per_chunk)
            self._prepare_minibatches(storage, T * E, N, K)
        if self.normalize_advantage:
            from . import _native
            self._std_ws_bytes = _native.workspace("dronesim_standardize_workspace", T * E, N)
            self._std_ws = torch.empty(self._std_ws_bytes // 8, dtype=torch.float64, device=dev)
            self.adv_stats = torch.zeros(2, N, device=dev)
        if self.target_kl is not None:
            self.active = torch.ones(N, dtype=torch.int32, device=dev)
            self.actor_steps = torch.zeros(N, dtype=torch.int32, device=dev)
        if self.obstacles is not None:
            _prepare_obstacles(self, storage, T, E, N)
        if self.obs_norm is not None:
            _prepare_obs_norm(self, storage)
        if self.reward_norm is not None:
            self._rn = torch.empty(T, E, N, device=dev)
        self._shape = (T, E, N)

    def _prepare_forms(self, critic_grad, actor_grad):
        """Grow the two runners' workspaces for the forms the epochs call, ahead of the first step."""
        actor_grad._workspace("grad_ppo")
        if self._ent:
            actor_grad._workspace("grad_ppo_gated" if self.target_kl is not None else "grad_ppo_ent")
        if self.vf_clip is not None:
            critic_grad._workspace("grad_vclip")

    def _prepare_minibatches(self, storage, rows, N, K):
        """The buffers of ``minibatches = K > 1``: the permutation, the five gathered arrays, the M-row gradient runners and the
        ``[epochs, K, ...]`` outputs."""
        import torch
        dev, M = self.critic.device, rows // K
        self.perm = torch.zeros(rows, dtype=torch.int32, device=dev)
        d = self.actor.d_in                                              # (the storage's width, plus the obstacle columns)
        shapes = ((N, d), (N, 2), (N,), (N,), (N,))                      # z_pre, actions, logp_old, adv, G
        if self.vf_clip is not None:
            shapes += ((N,),)                                            # and step 2's V, the clipped value loss's v_old
        n = len(shapes)
        self._mb = [GatheredRows(shape, K, M, dev) for shape in shapes]
        self._mb_dst = (C.c_void_p * n)(*[g.buf.data_ptr() for g in self._mb])
        self._mb_row_bytes = (C.c_int64 * n)(*[g.row_bytes for g in self._mb])
        self._mb_block_bytes = (C.c_int64 * n)(*[g.block_bytes for g in self._mb])
        self._critic_mb = GradientRunner(self.critic, M, self.rows_per_chunk)
        self._actor_mb = GradientRunner(self.actor, M, self.rows_per_chunk)
        self._prepare_forms(self._critic_mb, self._actor_mb)
        if self.vf_clip is not None:
            self._vclip = torch.zeros(self.epochs, K, N, device=dev)
        self._scalars = torch.zeros(4, self.epochs, K, N, device=dev)
        self._stats = torch.zeros(self.epochs, K, self._stat_rows, N, device=dev)

    def _train_minibatches(self, storage, x):
        """Step 3 with ``minibatches = K > 1``: per epoch a fresh device permutation, one gather, K critic-then-actor steps."""
        from . import _native
        T, E, N = self._shape
        K, rows = self.minibatches, T * E
        M = rows // K
        # (z_pre and actions are contiguous float32: step 2's forward-only pass has checked them)
        arrays = [x, storage.actions, self.logp_old, self.adv, self.G] + ([self.V] if self.vf_clip is not None else [])
        n_arrays = len(arrays)
        src = (C.c_void_p * n_arrays)(*[t.data_ptr() for t in arrays])
        for ep in range(self.epochs):
            _native.call("dronesim_row_permutation", rows, self.shuffle_seed, self.critic_opt.steps, self.perm, device=self.critic.device)
            _native.call("dronesim_gather_rows", self.perm, rows, M, n_arrays, src, self._mb_dst, self._mb_row_bytes, self._mb_block_bytes,
                         device=self.critic.device)
            for b in range(K):
                self._step(self._critic_mb, self._actor_mb, M, *(g.blocks[b] for g in self._mb), at=(ep, b),
                           last=ep == self.epochs - 1 and b == K - 1)
        return self._outputs()

    def _kl_gate(self, kl, reset):
        from . import _native
        share = self.actor_opt.share
        gate = (kl, self.target_kl, self.active, self.actor_steps, self.actor.n_agents, int(reset))
        if share is None:
            _native.call("dronesim_kl_gate", *gate, device=self.critic.device)
        else:       # the group's verdict, from the mean of its members' estimates, for all its members
            _native.call("dronesim_kl_gate_shared", *gate, share.group_ptr, share.members, share.n_groups, device=self.critic.device)

    def _step(self, critic_grad, actor_grad, rows, x, act, logp_old, adv, G, V=None, *, at, last):
        """One critic step, then one actor step, on these ``rows`` rows (the window, or one minibatch's block of every gathered
        array; ``V`` only with ``vf_clip``), results into slot ``at`` of the per-step outputs.  ``last``: re-pack the forward
        images.  Under ``target_kl`` the actor step is the gated gradient, the gate on this step's KL estimate, the gated Adam
        step."""
        closs, aloss, cnorm, anorm = (t[at] for t in self._scalars)
        if self.vf_clip is not None:
            cg = critic_grad.run_vclip(x, 1.0 / rows, G, V, self.vf_clip, loss_out=closs, clip_out=self._vclip[at])[0]
        else:
            cg = critic_grad.run(x, 1.0 / rows, target=G, loss_out=closs)[0]
        self.critic_opt.step(cg, norm_out=cnorm, refresh=last)
        ppo, out = (x, 1.0 / rows, act, logp_old, adv, self.clip_eps), dict(loss_out=aloss, stats_out=self._stats[at])
        if self.target_kl is not None:
            ag, _, st = actor_grad.run_ppo_gated(*ppo, self.ent_coef / rows, active=self.active, **out)
            self._kl_gate(st[5], False)
            self.actor_opt.step(ag, norm_out=anorm, refresh=last, active=self.active)
            return
        ag = (actor_grad.run_ppo_ent(*ppo, self.ent_coef / rows, **out) if self._ent else actor_grad.run_ppo(*ppo, **out))[0]
        self.actor_opt.step(ag, norm_out=anorm, refresh=last)

    def _outputs(self):
        """What ``train()`` returns, from the per-step buffers ``[epochs(, K), ...]``."""
        closs, aloss, cnorm, anorm = self._scalars
        st = self._stats
        out = dict(critic_loss=closs, actor_loss=aloss, critic_grad_norm=cnorm, actor_grad_norm=anorm,
                   clip_fraction=st[..., 0, :], approx_kl=st[..., 1, :], ratio_min=st[..., 2, :], ratio_max=st[..., 3, :])
        if self._ent:
            out["entropy"] = st[..., 4, :]
        if self.normalize_advantage:
            out.update(adv_mean=self.adv_stats[0], adv_std=self.adv_stats[1])
        if self.target_kl is not None:
            out.update(kl=st[..., 5, :], actor_steps=self.actor_steps)
        if self.vf_clip is not None:
            out["vf_clip_fraction"] = self._vclip
        return out

    def train(self, storage):
        from . import _native
        self._prepare(storage)
        T, E, N = self._shape
        act, nbr = storage.actions, storage.nbr_pre
        x, ring = _normalised(self, storage, T)
        reward = _normalised_reward(self, storage)
        if self.target_kl is not None:
            self._kl_gate(None, True)
        if self.lam is None:
            _native.call("dronesim_returns", reward, storage.done, self.gamma, self.G, T, E, N, device=self.critic.device)
        # the old policy's log-probabilities and the advantage from the pre-update critic, once per window (:484-501, :512-513)
        self._actor_grad.logp(x, act, self.logp_old)
        if self.lam is None:
            self.critic.forward(x.view(T * E, N, -1), out=self.V)
        else:       # the same forward over all T+1 ring slots; the bootstrapped lambda-returns of it
            self.critic.forward(ring.view((T + 1) * E, N, -1), out=self.V_all)
            (_lambda_returns if self.time_limit == "terminal" else _lambda_returns_ends)(self, storage, self.V_all, self.G, reward)
        _native.call("dronesim_neighbour_advantage", self.G, self.V, nbr, int(self.baseline == "per_neighbour"), self.adv, T, E, N,
                     int(nbr.shape[3]), device=self.critic.device)
        if self.normalize_advantage:
            _native.call("dronesim_standardize", self.adv, self.adv, self.adv_stats, T * E, N, self.adv_eps, self._std_ws,
                         self._std_ws_bytes, device=self.critic.device)
        if self.minibatches > 1:
            out = self._train_minibatches(storage, x)
        else:
            for ep in range(self.epochs):
                self._step(self._critic_grad, self._actor_grad, T * E, x, act, self.logp_old, self.adv, self.G, self.V, at=ep,
                           last=ep == self.epochs - 1)
            out = self._outputs()
        if self.obs_norm is not None and self.update_obs_norm:
            # the last enqueued work: the T E pre-step rows only (ring slot T is the next window's slot 0 and is counted there)
            self.obs_norm.update(_obs_norm_rows(self, storage, T))
        if self.reward_norm is not None:
            out["reward_scale"] = self.reward_norm.scale
        if self.obstacles is not None:
            out["obstacle_cost"] = self.obstacle_cost
        return out
