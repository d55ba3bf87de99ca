"""Per-agent learner step of the batched networks (SAC_agents.py:280-357, `SA2CAgents.train_NN`).

The reference trains its N actors and N critics one by one in Python, with torch autograd, once per episode.  Here the
N networks of a `BatchedMLP` are trained together by the HIP library (csrc/learner.hip, exact float32):

  mlp_gradients   dronesim_mlp_grad    per-agent loss gradients over all rows of a window, in one flat buffer
  BatchedAdam     dronesim_adam_step   clip_grad_norm_(max_norm) + torch.optim.Adam, per agent, in place on the weights
  SA2CLearner                          critic update, baseline from the post-update critic, actor update (train_NN)

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
    n = C.c_size_t(0)
    _native.check(_native.lib().dronesim_mlp_grad_workspace(C.byref(plain_struct(mlp)), int(rows_per_chunk), C.byref(n)),
                  "dronesim_mlp_grad_workspace")
    return int(n.value)


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
    """`dronesim_mlp_grad` for one network with its own persistent buffers: ``run()`` allocates nothing."""

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

    def run(self, x, row_scale, target=None, act=None, weight=None):
        import torch
        from . import _native
        mlp = self.mlp
        if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != self.rows * mlp.n_agents * mlp.d_in:
            raise ValueError(f"x must be a contiguous float32 tensor of {self.rows} rows x {mlp.n_agents} agents x {mlp.d_in}")
        per_row = {"target": (target, 1), "act": (act, 2), "weight": (weight, 1)}
        for name, (t, k) in per_row.items():
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.rows * mlp.n_agents * k):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {self.rows} x {mlp.n_agents} x {k}")
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(mlp.device):
            rc = _native.lib().dronesim_mlp_grad(C.byref(self._m), x.data_ptr(), self.rows, float(row_scale), ptr(target),
                                                 ptr(act), ptr(weight), self.grad.data_ptr(), self.loss.data_ptr(), self.rc,
                                                 self.ws.data_ptr(), self.ws_bytes,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, "dronesim_mlp_grad")
        return self.grad, self.loss


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


class BatchedAdam:
    """clip_grad_norm_(max_norm) + torch.optim.Adam (torch defaults: no weight decay, no amsgrad) for the N networks of
    one `BatchedMLP`, one optimiser state per agent: flat moments ``m1`` / ``m2`` and a per-agent step counter in device
    memory (a captured graph advances it on every replay).  ``step(grad)`` returns the pre-clip norms ``[N]``."""

    def __init__(self, mlp, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=10.0):
        import torch
        self.mlp = mlp
        self.lr, self.betas, self.eps, self.max_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(max_norm)
        _, total = flat_layout(mlp.n_agents, mlp.d_in, mlp.h1, mlp.h2, mlp.nout)
        self.numel = total
        self.m1 = torch.zeros(total, device=mlp.device)
        self.m2 = torch.zeros(total, device=mlp.device)
        self.steps = torch.zeros(mlp.n_agents, dtype=torch.int32, device=mlp.device)
        self.grad_norm = torch.zeros(mlp.n_agents, device=mlp.device)
        self._m = plain_struct(mlp)

    def step(self, grad):
        import torch
        from . import _native
        if grad.dtype != torch.float32 or not grad.is_contiguous() or grad.numel() != self.numel or grad.device != self.m1.device:
            raise ValueError(f"grad must be the flat float32 gradient buffer ({self.numel} elements) on {self.m1.device}")
        with torch.cuda.device(self.mlp.device):
            rc = _native.lib().dronesim_adam_step(C.byref(self._m), grad.data_ptr(), self.m1.data_ptr(), self.m2.data_ptr(),
                                                  self.steps.data_ptr(), self.lr, self.betas[0], self.betas[1], self.eps,
                                                  self.max_norm, self.grad_norm.data_ptr(),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, "dronesim_adam_step")
        self.mlp.refresh_weights()
        return self.grad_norm


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
    nothing after the first call" holds for the learner's buffers, not for those packing temporaries."""

    def __init__(self, actor, critic, gamma, lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0, rows_per_chunk=None):
        if critic.out_kind != 0 or critic.nout != 1:
            raise ValueError("the critic must be a BatchedMLP with out_kind 0 and one output")
        if actor.out_kind not in (1, 2):
            raise ValueError("the actor must be a softmax (out_kind 1) or Gaussian (out_kind 2) BatchedMLP")
        if (actor.n_agents, actor.d_in) != (critic.n_agents, critic.d_in):
            raise ValueError("actor and critic must have the same agents and inputs")
        self.actor, self.critic, self.gamma = actor, critic, float(gamma)
        self.rows_per_chunk = rows_per_chunk
        self.actor_opt = BatchedAdam(actor, lr=lr_actor, max_norm=max_norm)
        self.critic_opt = BatchedAdam(critic, lr=lr_critic, max_norm=max_norm)
        self._shape = None

    def _prepare(self, storage):
        import torch
        T, E, N = storage.reward.shape
        if self._shape == (T, E, N):
            return
        if N != self.critic.n_agents or storage.z_pre.shape[-1] != self.critic.d_in:
            raise ValueError("the storage's agents / observation width do not match the networks")
        if storage.actions is None:
            raise ValueError("the learner needs a storage with actions")
        dev = self.critic.device
        self.G = torch.empty(T, E, N, device=dev)
        self.V = torch.empty(T * E, N, 1, device=dev)
        self.w = torch.empty(T, E, N, device=dev)
        self._critic_grad = GradientRunner(self.critic, T * E, self.rows_per_chunk)
        self._actor_grad = GradientRunner(self.actor, T * E, self.rows_per_chunk)
        self._shape = (T, E, N)

    def train(self, storage):
        import torch
        from . import _native
        self._prepare(storage)
        T, E, N = self._shape
        lib, stream = _native.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
        x = storage.z_pre
        with torch.cuda.device(self.critic.device):
            rc = lib.dronesim_returns(storage.reward.data_ptr(), storage.done.data_ptr(), self.gamma, self.G.data_ptr(),
                                      T, E, N, stream)
        _native.check(rc, "dronesim_returns")
        # critic (SAC_agents.py:304-324)
        cg, closs = self._critic_grad.run(x, 1.0 / (T * E), target=self.G)
        cnorm = self.critic_opt.step(cg)
        # baseline from the post-update critic, advantage weights (:333-351)
        self.critic.forward(x.view(T * E, N, -1), out=self.V)
        nbr = storage.nbr_pre
        with torch.cuda.device(self.critic.device):
            rc = lib.dronesim_advantage(self.G.data_ptr(), self.V.data_ptr(), nbr.data_ptr(), storage.done.data_ptr(),
                                        self.gamma, self.w.data_ptr(), T, E, N, int(nbr.shape[3]), stream)
        _native.check(rc, "dronesim_advantage")
        # actor (:327-357)
        ag, aloss = self._actor_grad.run(x, 1.0 / E, act=storage.actions, weight=self.w)
        anorm = self.actor_opt.step(ag)
        return dict(critic_loss=closs, actor_loss=aloss, critic_grad_norm=cnorm, actor_grad_norm=anorm)
