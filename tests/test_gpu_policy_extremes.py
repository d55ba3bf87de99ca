"""The policy kernels at the edges of their LDS layouts: the named test for a kernel and a host that disagree about the layout (an LDS
access out of bounds, or a weight ring over the bias table -- failures an output comparison at ordinary shapes rarely names).  Run
with `-m gpu` on the MI355X box.

Per configuration of tests/helpers.py: POLICY_CONFIGS the accepted shapes with the largest and the smallest LDS of the recorded plan
(tests/test_policy_plan_host.py: extreme_shapes); for the two row-tile kernels both sides of the nout <= 4 switch (layer 3 on the vector
ALU from a table in LDS / on the matrix cores from the stream) at h1 = h2 = 512 with d_in at the family's cap; for bf16 NC1 = 8 and 9,
where the ring depth and the occupancy bound change.  N = 2 and E = one row block + 1: a second, ragged workgroup runs per agent.
`forward` against the float64 einsum at the bars of test_policy_shape_fuzz_all_precisions (2e-5 / 1e-5 max(1, |ref|); bf16 3e-2);
`sample_action` of one softmax and one Gaussian shape against tests/sampling_ref.py."""
import numpy as np
import pytest

from tests import helpers as H
from tests import sampling_ref as R
from tests.test_gpu_sampling import check_categorical, check_gaussian, policy
from tests.test_policy_plan_host import extreme_shapes

pytestmark = pytest.mark.gpu

N = 2
ROW_BLOCK = {"f32": 128, "f32-fragments": 32, "f32-w2-unpacked": 32, "bf16x3": 64, "f16x2": 128, "f16x2-split": 64, "bf16": 64}
RT_CAP = {"f32": 14, "f16x2": 16}                                # d_in caps of mlp3_rt_kernel / mlp3_rt16_kernel
CASES = ([(c, which, shape) for c, pair in extreme_shapes().items() for which, shape in zip(("largest-lds", "smallest-lds"), pair)]
         + [(c, f"nout-{nout}", (RT_CAP[c], 512, 512, nout)) for c in RT_CAP for nout in (4, 5)]
         + [("bf16", f"nc1-{nc1}", (6, h1, 64, 16)) for nc1, h1 in ((8, 256), (9, 257))])


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def test_extreme_shapes_are_the_plans():
    """(what the cases above rest on: the largest tiles are the families' caps, the smallest the 1-1-1-1 network)"""
    ext = extreme_shapes()
    assert set(ext) == set(H.POLICY_CONFIGS) == set(ROW_BLOCK)
    assert all(pair[1][1:3] == (1, 1) for pair in ext.values())
    assert ext["f16x2"][0][1:3] == (512, 512) and ext["f32-fragments"][0][:2] == (64, 512) and ext["bf16"][0][1] == 512


@pytest.mark.parametrize("config,which,shape", CASES, ids=[f"{c}-{w}" for c, w, _ in CASES])
def test_forward_at_the_edges_of_the_lds_layout(torch, config, which, shape):
    d, h1, h2, nout = shape
    E = ROW_BLOCK[config] + 1
    rng = np.random.default_rng([d, h1, h2, nout])
    w = R._network(rng, N, d, h1, h2, nout)
    x = (rng.uniform(-3.0, 3.0, (E, N, d))).astype(np.float32)
    kind = 1 if nout > 1 else 0                                  # softmax where it says something, else the plain output
    y = R.host_logits(w, x)
    ref = y if kind == 0 else R.host_softmax(w, x)
    pol = policy(config, w, kind, 0, 1)
    out = pol.forward(torch.from_numpy(x).cuda()).detach().cpu().numpy()
    tag = f"{config} {which} d={d} h1={h1} h2={h2} nout={nout} E={E}"
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(out - ref).max())
    print(f"\n{tag}: max |out - ref| = {err:.3e}, |ref| <= {np.abs(ref).max():.3e}")
    if config == "bf16":
        H.assert_close(out, ref, tag, rtol=3e-2, atol=3e-2 * scale)
    else:
        H.assert_close(out, ref, tag, rtol=2e-5, atol=1e-5 * scale)


def test_sampling_at_the_edges_of_the_lds_layout(torch):
    """nout = 5 on mlp3_rt_kernel (softmax, categorical) and nout = 4 on mlp3_rt16_kernel (Gaussian), h1 = h2 = 512, E = 129."""
    c = R.softmax_case("ordinary", 5, N, 129, d=14, h1=512, h2=512)
    pol = policy("f32", c["w"], 1, 1, c["seed"])
    _, _, ok = check_categorical(torch, pol, torch.from_numpy(c["x"]).cuda(), c["counter"], c["env_base"], "f32: " + c["tag"], per_case_cap=False)
    assert ok.mean() >= 0.99
    c = R.gaussian_case(N, 129, d=16, h1=512, h2=512)
    pol = policy("f16x2", c["w"], 2, 2, c["seed"])
    check_gaussian(torch, pol, torch.from_numpy(c["x"]).cuda(), c["counter"], c["env_base"], "f16x2: " + c["tag"])
