"""Gradients of composed shapes against the float64 duals of grad_f64.py, and the reference's own test.

  1. grad_f64.py alone (no product code): its duals against float64 central differences on random smooth expressions, its conventions at
     the non-differentiable points, its .vm reader and its matrix transform.
  2. eval_grad_slice of random shapes, prospero.vm, bear.vm and a gyroid, each seen through an affine, a rotated and a perspective matrix
     folded into the expression, on the oracle and (-m gpu) on the device.
  3. The normals of a 3D render (the voxel above the hit, through the screen -> model matrix and its division by w) on both back ends, and
     the gradients the mesher stores with its leaf samples (k_mesh_grads on the device), against the f64 gradient at the same points.

The measure is |g32 - g64|_inf / max(|g64|_inf, 1).  Its bound per shape and matrix is 4 x what the CPU oracle showed when
tests/golden/grad_f64_bounds.json was written (`python tests/test_grad_f64.py` rewrites it): the device is bit-equal to the oracle, so the
factor only absorbs another host's libm, while a wrong derivative rule moves the measure by orders of magnitude.  A point is left out when
the f64 reference alone finds it within TOL of a tie or a step (min, max, abs, floor, ceil, round, modulo, compare, and, or) - at most 1 % of a
shape's points.
"""
import json
import os
import random

import numpy as np
import pytest

import grad_f64 as G
from conftest import model_path
from test_render_random import build, build_full

TOL = 1e-4
N_POINTS = 2000
BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_f64_bounds.json")


# ---- 1. the reference itself ----------------------------------------------------------------------------------------------------
def smooth(rec, rng, depth):
    """a random expression of smooth operations, each kept inside its domain with bounded derivatives"""
    if depth == 0:
        a = rng.choice([rec.x, rec.y, rec.z])()
        return rec.add(rec.mul(a, rng.uniform(0.5, 1.5)), rng.uniform(-0.5, 0.5))
    a, b = smooth(rec, rng, depth - 1), smooth(rec, rng, depth - 1)
    k = rng.randrange(12)
    if k == 0: return rec.add(a, b)
    if k == 1: return rec.sub(a, b)
    if k == 2: return rec.mul(rec.sin(a), rec.cos(b))
    if k == 3: return rec.sin(rec.add(a, b))
    if k == 4: return rec.exp(rec.mul(rec.sin(a), 0.5))
    if k == 5: return rec.atan(rec.mul(a, b))
    if k == 6: return rec.sqrt(rec.add(rec.square(a), rec.add(rec.square(b), 1.0)))
    if k == 7: return rec.ln(rec.add(rec.square(a), 2.0))
    if k == 8: return rec.div(a, rec.add(rec.square(b), 2.0))
    if k == 9: return rec.atan2(rec.sin(a), rec.add(rec.cos(b), 2.5))
    if k == 10: return rec.recip(rec.add(rec.square(a), 1.5))
    return rec.mul(rec.tan(rec.mul(rec.sin(a), 0.5)), rec.add(rec.asin(rec.mul(rec.sin(b), 0.5)), rec.acos(rec.mul(rec.cos(a), 0.5))))


@pytest.mark.parametrize("seed", range(12))
def test_f64_duals_against_central_differences(seed):
    """d f / d axis by the duals against (f(p + h e) - f(p - h e)) / 2h in float64.

    Step and bound: the central difference is off by h^2 / 6 * |f'''| (truncation) + eps * |f| / h (rounding, eps = 2.2e-16).  The
    expressions are three levels of operations whose first three derivatives stay below ~10 on the reachable range (arguments of tan, asin,
    acos within +-0.5, denominators >= 1.5), over inputs in [-1, 1]: |f| < 1e2 and, by the chain rule through three levels, |f'''| < 1e5.
    With h = 1e-5: 1e-10 / 6 * 1e5 + 2.2e-16 * 1e2 / 1e-5 < 2e-6 + 3e-9.  The bound is 1e-5 * max(1, |d|); a wrong rule is off by O(|d|)."""
    rng = random.Random(seed)
    rec = G.Rec()
    root = smooth(rec, rng, 3)
    pts = np.random.default_rng(seed).uniform(-1, 1, (200, 3)).astype(np.float32).astype(np.float64)
    h = 1e-5

    def at(p):
        ins = {k: G.D(p[:, k], np.eye(3)[k][None, :].repeat(len(p), 0)) for k in range(3)}
        return G.evaluate(rec, root, ins)[0]
    d = at(pts)
    assert np.isfinite(d.v).all() and np.isfinite(d.d).all()
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        fd = (at(pts + e).v - at(pts - e).v) / (2 * h)
        err = np.abs(fd - d.d[:, k]) / np.maximum(1.0, np.abs(d.d[:, k]))
        assert err.max() < 1e-5, f"seed {seed} axis {k}: {err.max()}"


def test_f64_conventions_at_the_kinks():
    """what calculus leaves open, as grad_f64.py states it (each with its grad.rs line there)"""
    one = lambda v, ax: G.D.seed([v], ax)
    r = G._unary("abs", one(0.0, 0), None)
    assert r.v[0] == 0 and list(r.d[0]) == [1, 0, 0]
    r = G._unary("abs", one(-2.0, 0), None)
    assert r.v[0] == 2 and list(r.d[0]) == [-1, 0, 0]
    for op in ("min", "max"):        # a tie takes the right-hand side; NaN has no partials
        r = G._binary(op, one(1.5, 0), one(1.5, 1), None)
        assert r.v[0] == 1.5 and list(r.d[0]) == [0, 1, 0]
        r = G._binary(op, one(np.nan, 0), one(1.5, 1), None)
        assert np.isnan(r.v[0]) and list(r.d[0]) == [0, 0, 0]
    assert list(G._binary("min", one(1.0, 0), one(2.0, 1), None).d[0]) == [1, 0, 0]
    assert list(G._binary("max", one(1.0, 0), one(2.0, 1), None).d[0]) == [0, 1, 0]
    assert list(G._binary("and", one(0.0, 0), one(2.0, 1), None).d[0]) == [1, 0, 0]     # a == 0: a
    assert list(G._binary("and", one(0.5, 0), one(2.0, 1), None).d[0]) == [0, 1, 0]
    assert list(G._binary("or", one(0.0, 0), one(2.0, 1), None).d[0]) == [0, 1, 0]      # a == 0: b
    assert list(G._binary("or", one(0.5, 0), one(2.0, 1), None).d[0]) == [1, 0, 0]
    for op, arg, want in [("floor", 1.5, 1), ("ceil", 1.5, 2), ("round", 2.5, 3), ("round", -2.5, -3), ("not", 0.0, 1), ("not", 3.0, 0)]:
        r = G._unary(op, one(arg, 0), None)
        assert r.v[0] == want and not r.d.any()
    r = G._binary("compare", one(1.0, 0), one(2.0, 1), None)
    assert r.v[0] == -1 and not r.d.any()
    # modulo: the least non-negative remainder, a' - b' * floor(a / b)
    r = G._binary("mod", one(5.5, 0), one(2.0, 1), None)
    assert r.v[0] == 1.5 and list(r.d[0]) == [1, -2, 0]
    r = G._binary("mod", one(-5.5, 0), one(2.0, 1), None)
    assert r.v[0] == 0.5 and list(r.d[0]) == [1, 3, 0]
    r = G._binary("mod", one(5.5, 0), one(-2.0, 1), None)
    assert r.v[0] == 1.5 and list(r.d[0]) == [1, 2, 0]
    # ... and the modulo rule is the derivative away from the steps: central differences in b
    a, b, h = 5.3, 1.7, 1e-6
    f = lambda bb: a - bb * np.floor(a / bb)
    r = G._binary("mod", one(a, 0), one(b, 1), None)
    assert abs((f(b + h) - f(b - h)) / (2 * h) - r.d[0][1]) < 1e-6


def test_f64_near_marks_ties_and_steps():
    rec = G.Rec()
    x, y = rec.x(), rec.y()
    root = rec.add(rec.min(x, y), rec.floor(rec.mul(x, 4.0)))
    xs = np.array([0.3, 0.3, 0.25 + 5e-6, 0.6], np.float32)
    ys = np.array([0.9, 0.3 + 5e-5, 0.9, 0.6], np.float32)
    near = G.evaluate(rec, root, G.seeds(xs, ys, 0 * xs), tol=TOL)[1]
    assert list(near) == [False, True, True, True]
    # a flag that sits at 0 is not near a step of and / or; one that crosses 0 is
    root = rec.and_(rec.max(rec.compare(x, 0.5), 0.0), y)
    assert not G.evaluate(rec, root, G.seeds(xs, ys, 0 * xs), tol=TOL)[1].any()
    root = rec.and_(rec.sub(x, 0.3), y)
    assert list(G.evaluate(rec, root, G.seeds(xs, ys, 0 * xs), tol=TOL)[1]) == [True, True, False, False]


def test_f64_xf_against_central_differences():
    """the transform (rows 0..2 over row 3) numerically and folded into an expression: the same duals, and both the derivative of
    p -> M p / w by central differences (rational of degree 1: |f'''| < 1e2 here, so h = 1e-5 leaves < 2e-9 + 2e-11 * |f|)"""
    m = np.array([0.9, 0.1, -0.2, 0.05, -0.1, 1.1, 0.3, -0.1, 0.2, -0.3, 0.8, 0.07, 0.1, -0.05, 0.3, 1.0], np.float32)
    pts = np.random.default_rng(5).uniform(-1, 1, (100, 3)).astype(np.float32)
    num = G.xf(m, pts[:, 0], pts[:, 1], pts[:, 2])
    rec = G.Rec()
    ax = G.xf_fold(rec, m)
    m64 = m.astype(np.float64).reshape(4, 4)

    def plain(p):
        q = np.c_[p, np.ones(len(p))] @ m64.T
        return q[:, :3] / q[:, 3:]
    h = 1e-5
    for i in range(3):
        folded = G.evaluate(rec, ax[i], G.seeds(pts[:, 0], pts[:, 1], pts[:, 2]))[0]
        assert np.abs(folded.v - num[i].v).max() < 1e-15 and np.abs(folded.d - num[i].d).max() < 1e-14
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            fd = (plain(pts.astype(np.float64) + e)[:, i] - plain(pts.astype(np.float64) - e)[:, i]) / (2 * h)
            assert np.abs(fd - num[i].d[:, k]).max() < 1e-7


def test_f64_reads_vm_text():
    text = "# a sphere\n_0 var-x\n_1 square _0\n_2 var-y\n_3 square _2\n_4 add _1 _3\n_5 sqrt _4\n_6 const 0.5\n_7 sub _5 _6\n"
    rec = G.Rec()
    root = G.read_vm(rec, text)
    r = G.evaluate(rec, root, G.seeds([3.0], [4.0], [0.0]))[0]
    assert r.v[0] == 4.5 and np.allclose(r.d[0], [0.6, 0.8, 0.0], rtol=1e-15)
    with pytest.raises(ValueError):
        G.read_vm(G.Rec(), "_0 var-x\n_1 frobnicate _0\n")


# ---- 2. composed shapes ------------------------------------------------------------------------------------------------------------
def rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def camera(perspective, scale=1 / 0.7):
    """roll 30 degrees about z, pitch 60 about x, `scale`, `perspective` at (3, 2): w = 1 + perspective * z"""
    cam = np.eye(4)
    cam[3, 2] = perspective
    return (rot(2, 30) @ rot(0, 60) @ np.diag([scale, scale, scale, 1.0]) @ cam).astype(np.float32)


# (the scales keep the image of [-1, 1]^3 inside [-1, 1]^3, where the models live: bear.vm's smooth minima leave float32's range outside it)
MATRICES = {
    "affine": np.array([0.9, 0, 0, 0.05, 0, 1.1, 0, -0.1, 0, 0, 0.8, 0.07, 0, 0, 0, 1], np.float32).reshape(4, 4),
    "rotated": camera(0.0, 0.55),
    "perspective": camera(0.3, 0.4),
}
RENDER_CAMERA = camera(0.3)


def gyroid(ctx):
    """a gyroid shell of period 1/3 inside a sphere"""
    x, y, z = (ctx.mul(a, 6.0 * np.pi / 2) for a in (ctx.x(), ctx.y(), ctx.z()))
    g = ctx.add(ctx.add(ctx.mul(ctx.sin(x), ctx.cos(y)), ctx.mul(ctx.sin(y), ctx.cos(z))), ctx.mul(ctx.sin(z), ctx.cos(x)))
    shell = ctx.sub(ctx.abs(g), 0.3)
    r = ctx.sub(ctx.sqrt(ctx.add(ctx.add(ctx.square(ctx.x()), ctx.square(ctx.y())), ctx.square(ctx.z()))), 0.95)
    return ctx.max(shell, r)


def vm(name):
    def make(ctx):
        with open(model_path(name)) as f:
            return G.read_vm(ctx._rec if isinstance(ctx, G.View) else ctx, f.read(), axes=(ctx.x(), ctx.y(), ctx.z()))
    return make


SHAPES = {
    **{f"random{seed}": (lambda ctx, seed=seed: build(ctx, seed)) for seed in (0, 1, 2, 3)},
    **{f"every_opcode{seed}": (lambda ctx, seed=seed: build_full(ctx, seed)) for seed in (0, 1, 2)},
    "prospero": vm("prospero.vm"),
    "bear": vm("bear.vm"),
    "gyroid": gyroid,
}
POINT_SEED = {}   # shape -> seed of its points, where the default (the shape's position in SHAPES) left more than 1 % of them near a tie


def record(be, shape, matrix=None):
    """`shape` on the backend `be` (None: nowhere) and in a recorder, seen through `matrix`: (recorder, root)"""
    rec = G.Rec(be.Context() if be is not None else None)
    ctx = rec
    if matrix is not None:
        ctx = G.View(rec, G.xf_fold(rec, matrix))
    return rec, SHAPES[shape](ctx)


def points(shape):
    seed = POINT_SEED.get(shape, list(SHAPES).index(shape))
    return np.random.default_rng(seed).uniform(-1, 1, (N_POINTS, 3)).astype(np.float32)


def compare(g32, ref, near):
    """-> (the largest measure over the points kept, share of points left out).  Where the reference has no finite gradient (NaN from a
    hash or a domain), the result must have none either, and the point has no measure."""
    g32 = np.asarray(g32, np.float64)
    nan64 = ~np.isfinite(ref.v) | ~np.isfinite(ref.d).all(axis=1)
    keep = ~near & ~nan64
    nan32 = ~np.isfinite(g32).all(axis=1)
    assert (nan32[~near] == nan64[~near]).all(), f"{(nan32[~near] != nan64[~near]).sum()} points finite on one side only"
    m = G.measure(g32[keep, 1:4], ref.d[keep])
    mv = np.abs(g32[keep, 0] - ref.v[keep]) / np.maximum(np.abs(ref.v[keep]), 1.0)
    return float(max(m.max(), mv.max())), float(near.mean())


def measure_shape(be, shape, matrix):
    rec, root = record(be, shape, MATRICES[matrix])
    p = points(shape)
    ref, near = G.evaluate(rec, root, G.seeds(p[:, 0], p[:, 1], p[:, 2]), tol=TOL)
    got = be.Shape(rec.ctx, root.be).eval_grad_slice(p[:, 0], p[:, 1], p[:, 2])
    return compare(got, ref, near)


def bounds():
    with open(BOUNDS_PATH) as f:
        return json.load(f)["bounds"]


@pytest.mark.parametrize("matrix", list(MATRICES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_composed_gradients(be, shape, matrix):
    worst, left_out = measure_shape(be, shape, matrix)
    bound = 4 * bounds()[f"{shape}/{matrix}"]["measure"]
    print(f"{shape}/{matrix}: measure {worst:.3e} (bound {bound:.3e}), {100 * left_out:.2f} % of the points left out")
    assert left_out <= 0.01, f"{100 * left_out:.2f} % of the points are near a tie or a step"
    assert worst <= bound, f"{shape}/{matrix}: {worst:.3e} > {bound:.3e}"


# ---- 3. the renderer's normals and the mesher's gradients -------------------------------------------------------------------------------
RENDER_SIZE = 64


@pytest.mark.parametrize("shape", ["gyroid", "bear"])
def test_render_normals_under_perspective(be, shape):
    """normal = the gradient at the voxel above the hit, (px, py, depth - 1) seeded with the identity and taken through
    world_to_model * screen_to_world with its division by w (voxel.rs:412-450)"""
    rec, root = record(be, shape)
    w2m = RENDER_CAMERA
    img = be.render3d(be.Shape(rec.ctx, root.be), RENDER_SIZE, world_to_model=w2m)[0]
    py, px = np.nonzero((img["depth"] > 0) & (img["depth"] < RENDER_SIZE))
    assert len(px) > 500
    mat = be.mat_mul(w2m, be.screen_to_world([RENDER_SIZE] * 3))
    ax = G.xf(mat, px.astype(np.float32), py.astype(np.float32), (img["depth"][py, px] - 1).astype(np.float32))
    ref, near = G.evaluate(rec, root, {0: ax[0], 1: ax[1], 2: ax[2]}, tol=TOL)
    n = img["normal"][py, px].astype(np.float64)
    keep = ~near & np.isfinite(ref.d).all(axis=1)
    worst = float(G.measure(n[keep], ref.d[keep]).max())
    bound = 4 * bounds()[f"{shape}/perspective"]["measure"]
    print(f"{shape} normals: measure {worst:.3e} (bound {bound:.3e}), {len(px)} pixels, {100 * near.mean():.2f} % left out")
    assert near.mean() <= 0.01
    assert np.isfinite(n[keep]).all()
    assert worst <= bound


MESH_DEPTH = 5


def leaf_samples(be, shape):
    """the edge crossings the mesher sampled at its leaves: (positions [n, 3], {dx, dy, dz, value} [n, 4]).  The device's come from
    mesh_sample (k_mesh_grads), the oracle's from its octree."""
    if hasattr(be, "mesh_sample"):
        leaves = be.mesh_sample(shape, MESH_DEPTH)[0]
        n_edges, pos, grad = leaves["n_edges"], leaves["pos"], leaves["grad"]
    else:
        sm = be.Octree(shape, MESH_DEPTH).samples
        n_edges, pos, grad = sm["info"][:, 1], sm["pos"], sm["grad"]
    used = np.arange(12)[None, :] < n_edges[:, None]
    return pos[used], grad[used]


@pytest.mark.parametrize("shape", ["gyroid", "bear"])
def test_mesh_leaf_gradients(be, shape):
    """the gradient the mesher stores with each edge crossing of a leaf against the f64 gradient at the same model point"""
    rec, root = record(be, shape)
    pos, grad = leaf_samples(be, be.Shape(rec.ctx, root.be))
    assert len(pos) > 5000
    ref, near = G.evaluate(rec, root, G.seeds(pos[:, 0], pos[:, 1], pos[:, 2]), tol=TOL)
    keep = ~near & np.isfinite(ref.d).all(axis=1)
    worst = float(G.measure(grad[keep, :3], ref.d[keep]).max())
    bound = 4 * bounds()[f"{shape}/affine"]["measure"]
    print(f"{shape} mesh gradients: measure {worst:.3e} (bound {bound:.3e}), {len(pos)} samples, {100 * near.mean():.2f} % left out")
    assert near.mean() <= 0.01
    assert np.isfinite(grad[keep]).all()
    assert worst <= bound


# ---- one-opcode expressions seen through a projective matrix (the assembly normals interpreter's cases, tests/test_emu_normals.py) -----------
ONE_OP_IMM = 0.75
# (an immediate first only where the Context keeps it there: the commutative opcodes put it second, and / or fold it away)
ONE_OP_CASES = ([(n, "r") for n in G.UNARY] + [(n, f) for n in G.BINARY for f in ("rr", "ri")]
                + [(n, "ir") for n in ("sub", "div", "atan2", "compare", "mix", "mod")])


def one_op_build(ctx, name, form):
    x, y = ctx.x(), ctx.y()
    fn = getattr(ctx, G._PY.get(name, name))
    return fn(x) if form == "r" else fn(x, y) if form == "rr" else fn(x, ONE_OP_IMM) if form == "ri" else fn(ONE_OP_IMM, x)


def one_op_points(size=16):
    """every pixel of a size^2 image at a depth of its own: (px, py, pz = depth - 1) as float32"""
    py, px = np.mgrid[0:size, 0:size]
    px, py = px.ravel(), py.ravel()
    depth = 1 + (px * 7 + py * 3) % (size - 1)
    return px.astype(np.float32), py.astype(np.float32), (depth - 1).astype(np.float32), depth


def one_op_reference(name, form, mat, px, py, pz):
    """-> (f64 duals of the opcode at xf(mat, pixel), points to leave out).  Left out: within TOL of the opcode's tie or step, and where
    the operands are close to a pole or the edge of the domain - there the measure reports the conditioning of the function (an error of
    the transformed coordinate times f''), not the rule: |denominator| < 1/4 (recip, div, atan2's x^2 + y^2 < 1/16), argument < 1/4 (sqrt,
    ln), |argument| > 0.9 (asin, acos), |cos| < 1/4 (tan)."""
    rec = G.Rec()
    ax = G.xf_fold(rec, mat)
    root = one_op_build(G.View(rec, ax), name, form)
    ins = G.seeds(px, py, pz)
    ref, near = G.evaluate(rec, root, ins, tol=TOL)
    a = G.evaluate(rec, ax[0], ins)[0].v
    b = G.evaluate(rec, ax[1], ins)[0].v if form == "rr" else np.full(len(a), ONE_OP_IMM)
    if form == "ir":
        a, b = b, a
    risky = {"recip": np.abs(a) < 0.25, "sqrt": a < 0.25, "ln": a < 0.25, "asin": np.abs(a) > 0.9, "acos": np.abs(a) > 0.9,
             "tan": np.abs(np.cos(a)) < 0.25, "div": np.abs(b) < 0.25, "atan2": a * a + b * b < 0.0625}.get(name)
    return ref, (near | risky if risky is not None else near)


def one_op_bound(name, form):
    return 4 * bounds()[f"one_op/{name}_{form}"]["measure"]


def measure_one_op(be, name, form, mat):
    px, py, pz, _ = one_op_points()
    ref, skip = one_op_reference(name, form, mat, px, py, pz)
    rec = G.Rec(be.Context())
    root = one_op_build(G.View(rec, G.xf_fold(rec, mat)), name, form)
    got = np.asarray(be.Shape(rec.ctx, root.be).eval_grad_slice(px, py, pz), np.float64)
    keep = ~skip & np.isfinite(ref.v) & np.isfinite(ref.d).all(axis=1)
    assert keep.sum() >= 50, (name, form, int(keep.sum()))
    return float(G.measure(got[keep, 1:4], ref.d[keep]).max())


@pytest.mark.parametrize("name,form", ONE_OP_CASES)
def test_one_op_through_a_perspective_matrix(be, name, form):
    """eval_grad_slice of op(xf(pixel)) - the expression the normals kernels evaluate for a one-opcode tape - within its bound"""
    from test_emu_columns import PERSPECTIVE
    worst = measure_one_op(be, name, form, PERSPECTIVE)
    print(f"{name} {form}: {worst:.3e} (bound {one_op_bound(name, form):.3e})")
    assert worst <= one_op_bound(name, form)


# ---- the bounds file --------------------------------------------------------------------------------------------------------------------
def write_bounds():
    import oracle
    import fidget_amd
    n, first = fidget_amd.libm_probe()
    probe = ("this host's libm is the one the device restates (0 of 288 probe arguments differ)" if n == 0
             else f"{n} of 288 probe arguments differ, first {first}")
    out = {"libm_probe": probe, "tol": TOL, "points": N_POINTS, "backend": "CPU oracle", "bounds": {}}
    for shape in SHAPES:
        for matrix in MATRICES:
            worst, left_out = measure_shape(oracle, shape, matrix)
            out["bounds"][f"{shape}/{matrix}"] = {"measure": float(f"{worst:.3e}"), "left_out": round(left_out, 4)}
            print(shape, matrix, out["bounds"][f"{shape}/{matrix}"], flush=True)
    from test_emu_columns import PERSPECTIVE
    for name, form in ONE_OP_CASES:
        # (an opcode whose partials are exact - a selection, a constant - measures 0; the smallest bound is one float32 rounding of the
        # transformed coordinate's partials, 2^-24)
        out["bounds"][f"one_op/{name}_{form}"] = {"measure": float(f"{max(measure_one_op(oracle, name, form, PERSPECTIVE), 2.0 ** -24):.3e}")}
    with open(BOUNDS_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    write_bounds()
