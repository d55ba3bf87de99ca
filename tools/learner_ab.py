#!/usr/bin/env python3
"""Bit-for-bit A/B of the learner's native entry points between two builds of libdronesim.so, for refactorings of
csrc/learner.hip / csrc/standardize.hip that claim "same results".  Two runs, two processes, the library chosen by DRONESIM_LIB:

    DRONESIM_LIB=before.so python tools/learner_ab.py --dump ab.npz
    DRONESIM_LIB=after.so  python tools/learner_ab.py --compare ab.npz

Every entry point runs once on seeded inputs and every output buffer is kept as its int32 bit patterns (so the NaN of a gated
agent equals itself); --compare requires equality of all of them and exits 1 otherwise.  The shapes are the smallest that reach
every branch: N = 3 agents, R = 200 rows in chunks of 64 (first chunk writes, two accumulate, the last has 8 rows and divides),
d_in = 7, h1 = 48, h2 = 80 (tile edges inside both hidden widths); a critic, a softmax actor (nout = 5; agent 2's last logit is
125 below the others: p = 0 in float32) and a Gaussian actor; advantages of both signs, logp_old off by up to +-0.5 (both clip
branches and unclipped rows), a vf_clip that clamps some rows, active = [1, 0, 1]."""
import argparse
import ctypes as C
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scalable_collision_avoidance_rl_amd import _native  # noqa: E402
from scalable_collision_avoidance_rl_amd.learner import TENSOR_NAMES, BatchedAdam, GradientRunner, tensor_shapes  # noqa: E402

N, R, RC, D, H1, H2 = 3, 200, 64, 7, 48, 80
DEV = "cuda:0"


def run_all():
    gen = torch.Generator().manual_seed(20240607)
    rnd = lambda *shape: (torch.rand(*shape, generator=gen) * 2 - 1).to(DEV)
    out = {}

    def keep(name, *tensors):
        torch.cuda.synchronize()
        for k, t in enumerate(tensors):
            out[f"{name}.{k}"] = t.detach().contiguous().view(torch.int32).cpu().numpy().copy()

    def net(kind, nout):
        w = {n: rnd(N, *s) / max(s[0], 1) ** 0.5 for n, s in zip(TENSOR_NAMES, tensor_shapes(D, H1, H2, nout))}
        return types.SimpleNamespace(n_agents=N, d_in=D, h1=H1, h2=H2, nout=nout, out_kind=kind, device=torch.device(DEV),
                                     refresh_weights=lambda: None, **w)

    x, act, adv, target, weight = rnd(R, N, D), rnd(R, N, 2), rnd(R, N), rnd(R, N), rnd(R, N)
    act = act / act.norm(dim=-1, keepdim=True)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)

    critic = net(0, 1)
    run = GradientRunner(critic, R, RC)
    keep("critic.grad", *run.run(x, 1.0 / R, target=target))
    keep("critic.vclip", *run.run_vclip(x, 1.0 / R, target, rnd(R, N) * 0.5, 0.2))
    opt = BatchedAdam(critic, lr=1e-2, max_norm=0.05)
    weights = [getattr(critic, n) for n in TENSOR_NAMES]
    keep("adam", opt.step(run.grad), run.grad, opt.m1, opt.m2, opt.steps, *weights)
    keep("adam_gated", opt.step(run.grad, active=active), run.grad, opt.m1, opt.m2, opt.steps, *weights)

    for label, actor in (("softmax", net(1, 5)), ("gauss", net(2, 4))):
        if label == "softmax":
            actor.w3[2, :, 4] = 0.0
            actor.b3[2, 4] = -125.0
        run, logp = GradientRunner(actor, R, RC), torch.zeros(R, N, device=DEV)
        keep(label + ".grad", *run.run(x, 0.25, act=act, weight=weight))
        keep(label + ".logp", run.logp(x, act, logp))
        ppo = (x, 1.0 / R, act, logp + 0.5 * rnd(R, N), adv, 0.2)
        keep(label + ".ppo", *run.run_ppo(*ppo))
        keep(label + ".ent", *run.run_ent(x, 0.25, act, weight, 0.01 / R))
        keep(label + ".ppo_ent", *run.run_ppo_ent(*ppo, 0.01 / R))
        keep(label + ".gated_null", *run.run_ppo_gated(*ppo, 0.01 / R))
        keep(label + ".gated", *run.run_ppo_gated(*ppo, 0.01 / R, active=active))

    lib, taken = _native.lib(), torch.full((N,), 7, dtype=torch.int32, device=DEV)
    kl = torch.tensor([0.001, float("nan"), 0.5], device=DEV)
    for reset in (1, 0):
        _native.check(lib.dronesim_kl_gate(kl.data_ptr(), 0.01, active.data_ptr(), taken.data_ptr(), N, reset, None), "dronesim_kl_gate")
        keep(f"kl_gate.reset{reset}", active, taken)

    for rows, cols in ((200, 3), (128, 64)):
        v, n = rnd(rows, cols) * 3 - 500, C.c_size_t(0)
        _native.check(lib.dronesim_standardize_workspace(rows, cols, C.byref(n)), "dronesim_standardize_workspace")
        ws, y, stats = torch.empty(n.value // 8, dtype=torch.float64, device=DEV), torch.empty_like(v), torch.zeros(2, cols, device=DEV)
        _native.check(lib.dronesim_standardize(v.data_ptr(), y.data_ptr(), stats.data_ptr(), rows, cols, 1e-8, ws.data_ptr(), n.value,
                                               None), "dronesim_standardize")
        keep(f"standardize.{rows}x{cols}", y, stats)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--dump", metavar="FILE")
    mode.add_argument("--compare", metavar="FILE")
    args = ap.parse_args()
    out = run_all()
    if args.dump:
        with open(args.dump, "wb") as f:
            np.savez(f, **out)
        print(f"{len(out)} buffers of {_native.LIB_PATH} written to {args.dump}")
        return 0
    ref = np.load(args.compare)
    bad = [k for k in sorted(set(ref.files) | set(out)) if k not in out or k not in ref.files or not np.array_equal(ref[k], out[k])]
    for k in bad:
        n = int((ref[k] != out[k]).sum()) if k in out and k in ref.files and ref[k].shape == out[k].shape else -1
        print(f"MISMATCH {k}: {n} of {out[k].size if k in out else 0} words differ")
    print(f"{len(out) - len(bad)} of {len(out)} buffers of {_native.LIB_PATH} equal {args.compare} bit for bit, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
