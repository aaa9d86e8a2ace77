"""Cases and float64 references for the ray sampling and compositing kernels (csrc/raymarch.hip, csrc/composite.hip).

Truth is the oracle (oracle/lab4d_oracle.py) run on float64 tensors; `e_ref` is the float32 oracle's distance from it in the metric
the device is held to (relative L2, compared in float64 on the CPU).  Everything here runs without a GPU: tests/test_raypath_cases_cpu.py
re-asserts the reference's own error and the coverage of the case lists, tests/test_gpu_raypath.py runs the device against the same
(cached, never modified) references."""
import functools
from collections import namedtuple

import torch

from lab4d_amd.render_utils import KEY_FREEZE, KEY_MEAN, KEY_SKIP
from oracle import lab4d_oracle as O
from parity_report import NORTH_STAR_TOL

REF_FACTOR = 2.0      # parity_report.bound_of: twice the reference's own error ...
E_REF_MAX = 5e-5      # ... which stays below NORTH_STAR_TOL / 2 on every case, so the bound is 1e-4 throughout (asserted on the CPU)
KINDS = ("plain", "empty", "opaque", "noflow")
BAD_RAY = (0, 1)      # the ray the three degenerate kinds act on

CompositeCase = namedtuple("CompositeCase", "name M N D kind train")
RayCase = namedtuple("RayCase", "name M N D with_depth unit_q")


def _ccase(M, N, D, kind="plain", train=True):
    return CompositeCase("%s_%s_m%dn%dd%d" % (kind, "train" if train else "eval", M, N, D), M, N, D, kind, train)


COMPOSITE_CASES = (
    [_ccase(2, 5, D) for D in (1, 2, 63, 64, 65, 128, 129, 192, 193, 256)]
    + [_ccase(2, 5, D, train=False) for D in (65, 192)]
    + [_ccase(2, 5, D, kind) for kind in KINDS[1:] for D in (65, 193)]
    + [_ccase(1, 1, 129)]
)
WEIGHTS_D = (1, 65, 192, 256)
NULL_CASE = _ccase(2, 5, 65)
GRID_STRIDE_COMPOSITE = (1, 65541, 2)   # above 16384 blocks x 4 rays
GRID_STRIDE_RAYS = (1, 32800, 64)       # above 8192 blocks x 256 samples

RAY_CASES = [RayCase("m%dn%dd%d_%s_%s" % (M, N, D, "depth" if wd else "nearfar", "unit" if uq else "scaled"), M, N, D, wd, uq)
             for M, N, D, wd, uq in [(1, 1, 2, False, True), (3, 63, 3, True, True), (2, 64, 63, False, False), (2, 65, 64, True, False),
                                     (1, 129, 65, False, True), (2, 5, 129, True, False), (1, 300, 128, False, True)]]
NULL_RAY_CASE = RayCase("null", 2, 65, 65, False, False)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_l2(a, truth):
    """||a - truth|| / ||truth|| in float64 on the CPU (0 where both vanish)."""
    a, truth = a.detach().double().cpu(), truth.detach().double()
    n = float(truth.norm())
    d = float((a - truth).norm())
    return d / n if n > 0 else (0.0 if d == 0 else float("inf"))


def bound(e_ref):
    return max(NORTH_STAR_TOL, REF_FACTOR * e_ref)


# ---------------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------------


def composite_inputs(case):
    """float32 CPU leaves of one case, in field_dict order: aux5 | feature | aux7 alternate the generic-channel branch (LDS atomics) with
    the shuffle branch across consecutive fields."""
    M, N, D = case.M, case.N, case.D
    g = gen(1000 + 7 * D + 3 * M * N + KINDS.index(case.kind))
    r = lambda *c: torch.rand(M, N, D, *c, generator=g)
    n = lambda *c: torch.randn(M, N, D, *c, generator=g)
    fd = {"density": r(1) * 600.0 / D, "rgb": r(3), "vis": n(1) * 3, "xyz_cam": n(3), "eikonal": r(1), "gauss_density": r(1) * 200.0 / D}
    if case.train:
        fd.update({"flow_uv": n(2), "flow_valid": (r(1) > 0.3).float(), "aux2": n(2), "aux5": n(5), "feature": n(16), "aux7": n(7)})
    else:
        fd.update({"normal": n(3), "aux2": n(2), "aux5": n(5), "aux7": n(7)})
    deltas = r(1) * 0.02
    m, j = BAD_RAY
    if case.kind == "empty":
        fd["density"][m, j] = 0
        fd["gauss_density"][m, j] = 0
    elif case.kind == "opaque":
        fd["density"][m, j, : D // 4] = 1e4
    elif case.kind == "noflow":
        fd["flow_valid"][m, j] = 0
    fd["deltas"] = deltas
    return fd


def field_dict_of(leaves):
    """The reference-style field_dict over a dict of leaves (flow = cat(uv, validity); density_fg is density itself)."""
    fd = {}
    for k, v in leaves.items():
        if k in ("deltas", "flow_uv", "flow_valid"):
            continue
        fd[k] = v
        if k == "density":
            fd["density_fg"] = v
    if "flow_uv" in leaves:
        fd["flow"] = torch.cat([leaves["flow_uv"], leaves["flow_valid"]], -1)
    return fd


def composited_fields(case):
    """(key, channels, mode) of the fields the compositing kernels integrate for this case, in launch order (render_utils._composite)."""
    out = []
    for k, v in field_dict_of(composite_inputs(case)).items():
        if k in KEY_MEAN:
            out.append((k, v.shape[-1], 2))
        elif k not in KEY_SKIP:
            out.append((k, v.shape[-1], 1 if k in KEY_FREEZE else 0))
    return out


def channel_class(C):
    return "divides64" if 64 % C == 0 else ("three" if C == 3 else "generic")


def cotangents(out):
    """One random float64 cotangent per rendered key, the same for every implementation."""
    g = gen(99)
    return {k: torch.randn(out[k].shape, generator=g, dtype=torch.float64) for k in sorted(out)}


def run_render_pixel(render_pixel, inputs, dtype=torch.float32, device="cpu"):
    """render_pixel forward and backward -> (rendered, gradients of every leaf but the flow validity), detached."""
    leaves = {k: v.to(device=device, dtype=dtype).clone().requires_grad_(k != "flow_valid") for k, v in inputs.items()}
    out = render_pixel(field_dict_of(leaves), leaves["deltas"])
    loss = sum((out[k] * c.to(device=device, dtype=dtype)).sum() for k, c in cotangents(out).items())
    names = sorted(k for k in leaves if leaves[k].requires_grad)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])).detach() for k, g in zip(names, grads)}
    return {k: v.detach() for k, v in out.items()}, grads


def _tensors(out, grads):
    t = {"out." + k: v for k, v in out.items()}
    t.update({"grad." + k: v for k, v in grads.items()})
    return t


@functools.lru_cache(maxsize=None)
def composite_reference(case):
    """(truth64, ref32): name -> tensor for every output and gradient of the case.  Cached; callers must not modify it."""
    inputs = composite_inputs(case)
    return _tensors(*run_render_pixel(O.render_pixel, inputs, torch.float64)), _tensors(*run_render_pixel(O.render_pixel, inputs, torch.float32))


def weights_inputs(D, M=2, N=5):
    g = gen(2000 + D)
    return {"density": torch.rand(M, N, D, 1, generator=g) * 600.0 / D, "deltas": torch.rand(M, N, D, 1, generator=g) * 0.02,
            "cot": torch.randn(M, N, D, generator=g, dtype=torch.float64)}


def run_compute_weights(compute_weights, inputs, dtype=torch.float32, device="cpu"):
    dens = inputs["density"].to(device=device, dtype=dtype).clone().requires_grad_(True)
    dl = inputs["deltas"].to(device=device, dtype=dtype).clone().requires_grad_(True)
    w, T = compute_weights(dens, dl)
    gd, gl = torch.autograd.grad((w * inputs["cot"].to(device=device, dtype=dtype)).sum(), [dens, dl])
    return {"out.weights": w.detach(), "out.transmit": T.detach(), "grad.density": gd.detach(), "grad.deltas": gl.detach()}


@functools.lru_cache(maxsize=None)
def weights_reference(D):
    inputs = weights_inputs(D)
    return run_compute_weights(O.compute_weights, inputs, torch.float64), run_compute_weights(O.compute_weights, inputs, torch.float32)


# ---------------------------------------------------------------------------------------------------
# ray sampling
# ---------------------------------------------------------------------------------------------------

RAY_OUTPUTS = ("xyz_cam", "dir_cam", "deltas", "depth", "xyz_field", "dir_field")


def ray_inputs(case, with_cot=True):
    M, N, D = case.M, case.N, case.D
    g = gen(3000 + 11 * D + N + M)
    K = torch.tensor([[64.0, 0, 32], [0, 64, 32], [0, 0, 1]])[None].repeat(M, 1, 1)
    K[:, 0, 0] += torch.rand(M, generator=g) * 8
    K[:, 1, 1] += torch.rand(M, generator=g) * 8
    Kinv = (torch.linalg.inv(K) + torch.randn(M, 3, 3, generator=g) * 1e-3).contiguous()  # every entry of Kinv takes part
    near = 0.3 + 0.2 * torch.rand(M, generator=g)
    inp = {"hxy": torch.cat([torch.rand(M, N, 2, generator=g) * 64, torch.ones(M, N, 1)], -1), "Kinv": Kinv,
           "near_far": torch.stack([near, near + 0.3 + 0.2 * torch.rand(M, generator=g)], -1)}
    q = torch.nn.functional.normalize(torch.randn(M, 4, generator=g), dim=-1)
    if not case.unit_q:
        q = q * (0.7 + 0.6 * torch.rand(M, 1, generator=g))
    inp["cq"], inp["ct"] = q, torch.randn(M, 3, generator=g) * 0.1
    inp["depth"] = torch.sort(torch.rand(M, N, D, 1, generator=g) * 0.4 + 0.4, 2)[0] if case.with_depth else None
    if with_cot:
        inp["cot"] = [torch.randn(M, N, D, c, generator=g, dtype=torch.float64) for c in (3, 3, 1, 3, 3)]
    return inp


def oracle_ray_samples(hxy, Kinv, near_far, c2f, n_depth, depth=None):
    """The oracle's counterpart of render_utils.ray_samples: sample_cam_rays, then the rigid transform with the quaternion as given."""
    xyz, dirs, deltas, dep = O.sample_cam_rays(hxy, Kinv, near_far, n_depth=n_depth, depth=depth)
    q, t = O._expand_se3(c2f, xyz.shape)
    return xyz, dirs, deltas, dep, O.quaternion_translation_apply(q, t, xyz), O.quaternion_apply(q, dirs)


def run_ray_samples(fn, inp, D, dtype=torch.float32, device="cpu", depth=None):
    """fn(hxy, Kinv, near_far, (q, t), D, depth) -> the six outputs and the gradients of Kinv, q and t under the case's cotangents."""
    to = lambda t: t.to(device=device, dtype=dtype)
    K, q, t = (to(inp[k]).clone().requires_grad_(True) for k in ("Kinv", "cq", "ct"))
    depth = inp["depth"] if depth is None else depth
    outs = fn(to(inp["hxy"]), K, to(inp["near_far"]), (q, t), D, None if depth is None else to(depth))
    diff = [outs[i] for i in (0, 1, 2, 4, 5)]
    grads = torch.autograd.grad(sum((a * to(w)).sum() for a, w in zip(diff, inp["cot"])), [K, q, t])
    res = {"out." + k: v.detach() for k, v in zip(RAY_OUTPUTS, outs)}
    res.update({"grad." + k: v.detach() for k, v in zip(("Kinv", "cq", "ct"), grads)})
    return res


@functools.lru_cache(maxsize=None)
def ray_reference(case):
    """(truth64, ref32).  sample_cam_rays builds its linspace in float32: on the near_far path the float32 oracle's depth, upcast, is the
    float64 oracle's `depth=` input, so that both integrate the same sample positions."""
    inp = ray_inputs(case)
    ref32 = run_ray_samples(oracle_ray_samples, inp, case.D, torch.float32)
    truth = run_ray_samples(oracle_ray_samples, inp, case.D, torch.float64, depth=ref32["out.depth"])
    return truth, ref32


def run_cam_rays(fn, inp, D, dtype=torch.float32, device="cpu", depth=None):
    """The unfused path, fn(hxy, Kinv, near_far, D, depth) -> xyz_cam, dir_cam, deltas, depth: the four outputs and the gradient of Kinv."""
    to = lambda t: t.to(device=device, dtype=dtype)
    K = to(inp["Kinv"]).clone().requires_grad_(True)
    depth = inp["depth"] if depth is None else depth
    outs = fn(to(inp["hxy"]), K, to(inp["near_far"]), D, None if depth is None else to(depth))
    (gK,) = torch.autograd.grad(sum((a * to(w)).sum() for a, w in zip(outs[:3], inp["cot"])), [K])
    res = {"out." + k: v.detach() for k, v in zip(RAY_OUTPUTS, outs)}
    res["grad.Kinv"] = gK.detach()
    return res


def _oracle_cam_rays(hxy, Kinv, near_far, D, depth):
    return O.sample_cam_rays(hxy, Kinv, near_far, n_depth=D, depth=depth)


@functools.lru_cache(maxsize=None)
def cam_rays_reference(case):
    inp = ray_inputs(case)
    ref32 = run_cam_rays(_oracle_cam_rays, inp, case.D, torch.float32)
    return run_cam_rays(_oracle_cam_rays, inp, case.D, torch.float64, depth=ref32["out.depth"]), ref32


def sort_depth_cases():
    """(name, a, b): sorted runs as sample_pdf / linspace give them, plus the two rows that bound what the repair pass is relied on for."""
    out = []
    for i, (R, na, nb) in enumerate([(1, 1, 1), (257, 64, 1), (257, 1, 64), (300, 64, 16)]):
        g = gen(4000 + i)
        a = torch.sort(torch.rand(R, na, generator=g), -1)[0]
        b = torch.sort(torch.rand(R, nb, generator=g), -1)[0]
        if R > 1:
            a[3], b[3] = 0.5, 0.5                                        # every value of a equals every value of b
            if nb >= 8:
                b[5, 2:8] = torch.flip(b[5, 2:8].clone(), [-1])         # a descending run in b
        out.append(("r%d_a%d_b%d" % (R, na, nb), a, b))
    return out
