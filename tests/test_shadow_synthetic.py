"""The shadow stage on rays and triangles of its own: every cell row, edge-on hits, NaN and pole rays.

The stage is ugrt_map_rays_to_light -> ugrt_sort_rays -> ugrt_trace_shadow over the light grid of
ugrt_grid_build_spherical.  Every other shadow test feeds it the primary hits of a camera on cornell, hall or crash,
whose rays fall into two or three rows of light cells (the reference's getEffective_y multiplies where it should add,
orc_effective_y, so the row only spreads when the light's forward axis has one non-zero component) and lie on scene
surfaces.  Here the light looks along (1,0,0), so that the typo'd row expression spans every row, and the inputs are
built with numpy in float64, rounded once to float32, and seeded:

* triangles on shells around the light L: directions uniform on the sphere, distances log-uniform over two decades,
  sizes log-uniform from 0.3 % to 10 % of the distance, a handful that span many cells; one stack of 17 000 nearly
  coincident small triangles in a cell of its own (more than XSEG_LAST + 1 = 255 segments at "shadow_xseg" 64, so the
  last segment takes the rest); cells whose lists hold exactly 1, 63, 64, 65 and 129 triangles;
* rays, given as hit points P = cam_pos + t dir, of ten kinds dealt out at random per pixel:
   1 behind an interior point of a triangle k (expected flag 1)     2 in front of it
   3 on the line from L through a point of an edge of k, behind it  4 the same through a vertex of k
   5 behind an interior point at the occluder's distance + 0.5e-3, 1e-3, 2e-3 (isSmaller's epsilon)
   6 anywhere around L, radii log-uniform over 1e-3 .. 1e3          7 exactly on +-right, +-up, +-forward of the light
   8 P == L bit for bit (the light ray is 0/0)                      9 t = -1 and t = 0 (a miss is mapped and traced too)
  10 through the common interior of the stack, in front of it (undecided through all of its triangles)
  (7 and 8 need cam_pos + t dir exact in float32: t = 16 and dir = (P - cam_pos) / 16, all dyadic);
* incoming is_shadowed of 0, 1 and 7: the pass may only ever write 1.

Case A: image 256 x 128, light grid (32,16) = (W/8, H/8), which the reference's kernels can run too; case B: image
256 x 64, light grid (64,32).  Case C is sparse: image 64 x 64, light grid (512,256), rays of kinds 3 and 4 only, so
that nearly every ray is alone in its light cell.  Such a ray is a beam of its own whose direction box is the ray, and
the beam cull (k_shadow_boxes, k_shadow_cull, d_cull_decide) decides on the very edge the ray was aimed at with nothing
but its margins between its own rounding and the exact test's.

CPU tests (unmarked): conditions on the oracle alone that let the GPU tests fail (see test_inputs_can_fail).
GPU tests: the four stages against the oracle, integers and flags equal, in the waiting, deferred, all-chunks, band
and z-slab forms, and under every launch-shape option of the pass.  tests/golden/ref_kernels_shadowsyn.npz
(tests/golden/make_ref_kernels.py) records what the reference's own kernels compute on case A.

Oracle figures (every chunk traced unless said)                case A          case B
  triangles / light-grid references                            21 142 / 25 300 21 262 / 34 697
  light-grid cells used / rows / columns                       449 of 512 / 16 / 31   1 905 of 2 048 / 32 / 63
  distinct ray cells / rows                                    252 / 16        962 / 32
  longest cell list / most rays in one cell                    17 000 / 11 552 17 000 / 8 891
  chunks against launch blocks                                 638 / 512       1 136 / 256
  rays traced under the strict rule                            26 280          10 525
  traced, incoming flag not 1: shadowed / lit, strict          8 726 / 8 610   4 600 / 2 420
                                               every chunk     10 904 / 10 724 6 000 / 4 953
  edge and vertex rays shadowed / lit                          3 754 / 1 443   2 301 / 296
  occluder distance + 0.5e-3, 1e-3, 2e-3: shadowed / lit       349/376 462/241 723/16   261/95 312/61 328/12
  kind 1 with k in the ray's own list, all flagged 1           4 732           2 426
  flags changed by cutting every list at 64 entries            384             224
  ... by forcing every row to the commonest                    5 964           1 377
  ... by moving the edge and vertex rays by 1e-4               1 160           331
Case C (64 x 64, light grid (512,256), 4 000 triangles, R 632 359, 3 426 chunks): 2 575 edge and vertex rays are alone
in their cell with k in its list and an incoming flag other than 1; 1 486 of them shadowed, 1 089 lit; 878 / 887 of
their flags change when the rays move by 1e-6 / 1e-5.
Measured on an MI355X: the 37 GPU tests of this file take 2.5 s together (the slowest, the first to build case A, 0.3 s).
A build with the beam cull's margin K set to 0 and its boxes not widened (k_shadow_cull, k_shadow_boxes) fails
test_trace_strict[C] (6 flags) and test_trace_of_lone_edge_rays at every beam size (242 flags, 0 where the oracle has 1);
cases A and B alone do not see it, because few of their edge rays sit on a corner of their beam's box.
"""
import functools
import types

import numpy as np
import pytest

PI_F = float(np.float32(np.pi))
HALF_PI_F = float(np.float32(np.pi / 2))
TAIL = 64  # sentinel words behind a buffer the stage writes
SENT = 0xDEADBEEF
L = np.array([3.0, 4.0, 5.0])
CAM_POS = np.array([-7.0, 2.0, 11.0])  # L - CAM_POS = (10, 2, -6)
LIGHT = dict(eye=tuple(L), look=(4.0, 4.0, 5.0), up=(0.0, 1.0, 0.0), near=0.1, far=100.0)
FOVY = 45.0
CASES = {"A": (256, 128, (32, 16)), "B": (256, 64, (64, 32))}
SPARSE = (64, 64, (512, 256))  # case C: edge and vertex rays only, nearly every one alone in its light cell
BAND_ROWS = (4, 12)  # of case A's 16 tile rows
STACK = 17000  # >= 255 * 64 + 1 = 16 321
LIST_LENGTHS = (1, 63, 64, 65, 129)
XSEG_LAST = 254
# unit directions from L of the stack and of the cells with the list lengths above: kept clear of everything else
# (case B's lies in an early cell: the strict rule traces only the first 255 chunks of its 16 384 rays)
STACK_DIR = {"A": np.array([0.30, -0.50, 0.80]), "B": np.array([0.80, -0.50, -0.20])}
LIST_DIRS = np.array([[-0.60, 0.50, 0.40], [0.50, 0.60, -0.50], [-0.40, -0.60, -0.60], [0.70, -0.20, -0.60],
                      [-0.80, -0.30, 0.30]])
# share of the rays per kind 1..10, and of the rays of kinds 1..5 whose triangle k is one of the stack
KIND_SHARE = (0.22, 0.12, 0.14, 0.10, 0.10, 0.15, 0.012, 0.006, 0.04, 0.112)
STACK_SHARE = {"A": 0.40, "B": 0.80}
EPS_OFFSETS = (0.5e-3, 1e-3, 2e-3)
AXIS_STEPS = (0.5, 2.0, 8.0, 32.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def aspect_of(W, H):
    return float(np.float32(W) / np.float32(H))


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def cell_ranges(O, lcc, tris, lg):
    """[F, 4] (gxmin, gxmax, gymin, gymax) of the triangles' light cells, as the oracle's build bins them."""
    v = np.ascontiguousarray(tris.reshape(-1, 3), np.float32)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return O.grid_spherical(lcc, f, v, lg[0], lg[1])["rng"].reshape(-1, 4)


def one_cell(rng4, lg):
    """The cell of each triangle that lies in one cell, -1 for the others."""
    single = (rng4[:, 0] == rng4[:, 1]) & (rng4[:, 2] == rng4[:, 3])
    return np.where(single, rng4[:, 0] * lg[1] + rng4[:, 2], -1)


def covers(rng4, cells, lg):
    """Which triangles hold a reference in any of the cells."""
    hit = np.zeros(len(rng4), bool)
    for c in cells:
        cx, cy = c // lg[1], c % lg[1]
        hit |= (rng4[:, 0] <= cx) & (cx <= rng4[:, 1]) & (rng4[:, 2] <= cy) & (cy <= rng4[:, 3])
    return hit


@functools.lru_cache(maxsize=None)
def synthetic(O, case):
    """The inputs of a case: triangles, rays, incoming flags, and what each ray was built for."""
    if case == "C":
        return sparse(O)
    W, H, lg = CASES[case]
    N = W * H
    rng = np.random.default_rng(20261019 + ord(case))
    lcam = O.cam_from(LIGHT, FOVY, aspect_of(W, H))
    # -- triangles on shells around L
    ntri = 4000
    dist = np.exp(rng.uniform(np.log(0.5), np.log(50.0), ntri))
    size = dist * np.exp(rng.uniform(np.log(0.003), np.log(0.1), ntri))
    shells = (L + unit(rng.normal(size=(ntri, 3))) * dist[:, None])[:, None, :] + \
        rng.normal(size=(ntri, 3, 3)) * size[:, None, None]
    # a handful that span many cells: as wide as they are far
    nwide = 24
    wdist = np.exp(rng.uniform(np.log(2.0), np.log(30.0), nwide))
    wide = (L + unit(rng.normal(size=(nwide, 3))) * wdist[:, None])[:, None, :] + \
        rng.normal(size=(nwide, 3, 3)) * (0.5 * wdist)[:, None, None]
    # the stack: one small triangle, moved about by 3e-4
    base = (L + unit(STACK_DIR[case]) * 6.0)[None, :] + np.array([[0, 0, 0], [0.05, 0, 0], [0, 0.05, 0]])
    stack = base[None, :, :] + rng.normal(size=(STACK, 1, 3)) * 3e-4
    stack_cells = np.unique(one_cell(cell_ranges(O, lcam.cc, stack, lg), lg))
    # the cells with lists of a given length: tiny triangles around a direction, those that lie in its commonest cell
    lists, list_cells = [], []
    for d0, want in zip(LIST_DIRS, LIST_LENGTHS):
        r0 = rng.uniform(3.0, 12.0)
        cand = (L + unit(unit(d0) + rng.normal(size=(3000, 3)) * 0.01) * r0)[:, None, :] + \
            rng.normal(size=(3000, 3, 3)) * (0.002 * r0)
        cell = one_cell(cell_ranges(O, lcam.cc, cand, lg), lg)
        c = np.bincount(cell[cell >= 0]).argmax()
        lists.append(cand[cell == c][:want])
        list_cells.append(int(c))
    # ... and nothing else in these cells
    others = np.concatenate([shells, wide])
    others = others[~covers(cell_ranges(O, lcam.cc, others, lg), list(stack_cells) + list_cells, lg)]
    # triangles around the light's +-up and +-right: the poles of the mapping.  A point inside one can lie in a cell that
    # the box around its corners' cells does not hold, so the triangle is not in the list of a ray that hits it
    poles = []
    for axis in ((0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        a = np.asarray(axis, np.float64)
        e1 = np.array([1.0, 0.0, 0.0])
        e2 = np.cross(a, e1)
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
        poles.append(L + 5.0 * a + np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)
    first_pole = len(others)
    tris = np.concatenate([others, np.asarray(poles)] + lists + [stack])
    first_stack = len(tris) - STACK
    verts = np.ascontiguousarray(tris.reshape(-1, 3), np.float32)
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    v = verts.reshape(-1, 3, 3).astype(np.float64)
    # -- rays
    kind = rng.choice(np.arange(1, 11), N, p=np.asarray(KIND_SHARE) / np.sum(KIND_SHARE))
    k = np.where(rng.random(N) < STACK_SHARE[case], rng.integers(first_stack, len(tris), N),
                 rng.integers(0, first_stack, N))
    # (a share of them at the short lists, each list alike)
    to_list = np.flatnonzero(rng.random(N) < 0.06)
    which = rng.integers(0, len(LIST_LENGTHS), to_list.size)
    starts = first_pole + 4 + np.concatenate([[0], np.cumsum(LIST_LENGTHS)[:-1]])
    k[to_list] = starts[which] + rng.integers(0, 1 << 30, to_list.size) % np.asarray(LIST_LENGTHS)[which]
    to_pole = (kind == 5) & (rng.random(N) < 0.15)
    k[to_pole] = first_pole + rng.integers(0, 4, int(to_pole.sum()))
    inner = 0.15 + 0.55 * rng.dirichlet([1, 1, 1], N)  # barycentrics well inside
    b = inner.copy()
    edge = np.flatnonzero(kind == 3)
    pair = rng.dirichlet([1, 1], edge.size)
    zero = rng.integers(0, 3, edge.size)
    for j in range(3):
        sel = zero == j
        b[edge[sel]] = np.insert(pair[sel], j, 0.0, axis=1)
    corner = kind == 4
    b[corner] = np.eye(3)[rng.integers(0, 3, int(corner.sum()))]
    ten = kind == 10
    k[ten] = rng.integers(first_stack, len(tris), int(ten.sum()))
    b[ten] = 1.0 / 3.0 + rng.uniform(-0.1, 0.1, (int(ten.sum()), 3)) * [1, -1, 0]
    Q = (v[k] * b[:, :, None]).sum(1)
    fac = rng.uniform(1.01, 3.0, N)
    fac[kind == 2] = rng.uniform(0.3, 0.99, int((kind == 2).sum()))
    fac[ten] = rng.uniform(0.3, 0.9, int(ten.sum()))
    P = L + (Q - L) * fac[:, None]
    five = kind == 5
    offset = rng.integers(0, 3, N)
    dQ = np.linalg.norm(Q - L, axis=1)
    P[five] = (L + (Q - L) / dQ[:, None] * (dQ + np.asarray(EPS_OFFSETS)[offset])[:, None])[five]
    six = kind == 6
    P[six] = L + unit(rng.normal(size=(int(six.sum()), 3))) * \
        np.exp(rng.uniform(np.log(1e-3), np.log(1e3), int(six.sum())))[:, None]
    nine = kind == 9
    P[nine] = CAM_POS + unit(rng.normal(size=(int(nine.sum()), 3)))  # (their direction; t is set below)
    d = P - CAM_POS
    t = np.linalg.norm(d, axis=1)
    t[t == 0] = 1.0
    dirs = d / t[:, None]
    t[nine] = np.where(rng.random(int(nine.sum())) < 0.5, -1.0, 0.0)
    # kinds 7 and 8: cam_pos + 16 dir is exact in float32, so P lies on the axis, or is L, bit for bit
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    seven = np.flatnonzero(kind == 7)
    variant = rng.integers(0, 24, seven.size)
    variant[:24] = rng.permutation(24)  # each of the 24 at least once
    P[seven] = L + axes[variant % 6] * np.asarray(AXIS_STEPS)[variant // 6][:, None]
    axis = np.full(N, -1)
    axis[seven] = variant % 6  # +forward, +up, +right, -forward, -up, -right (the view looks along -forward)
    eight = kind == 8
    P[eight] = L
    exact = (kind == 7) | eight
    t[exact] = 16.0
    dirs[exact] = (P[exact] - CAM_POS) / 16.0
    t32, dirs32 = t.astype(np.float32), np.ascontiguousarray(dirs.astype(np.float32).reshape(-1))
    back = np.float32(CAM_POS)[None, :] + t32[exact, None] * dirs32.reshape(-1, 3)[exact]
    assert back.dtype == np.float32 and (back == P[exact]).all()
    flags = rng.choice(np.array([0, 1, 7], np.int32), N)
    return types.SimpleNamespace(case=case, W=W, H=H, lg=lg, N=N, C=lg[0] * lg[1], lcam=lcam, verts=verts, faces=faces,
                                 F=len(faces), first_stack=first_stack, stack_cells=stack_cells, list_cells=list_cells,
                                 nwide=nwide, kind=kind, axis=axis, k=k, offset=offset, t=t32, dirs=dirs32, flags=flags,
                                 cam_pos=CAM_POS.astype(np.float32))


def sparse(O):
    """Case C.  A ray that is alone in its light cell is a beam of its own, whose direction box is the ray: the beam
    cull then decides on the edge the ray was aimed at with nothing but its margins between it and the exact test."""
    W, H, lg = SPARSE
    N = W * H
    rng = np.random.default_rng(20261020)
    lcam = O.cam_from(LIGHT, FOVY, aspect_of(W, H))
    ntri = 4000
    dist = np.exp(rng.uniform(np.log(0.5), np.log(50.0), ntri))
    size = dist * np.exp(rng.uniform(np.log(0.003), np.log(0.1), ntri))
    tris = (L + unit(rng.normal(size=(ntri, 3))) * dist[:, None])[:, None, :] + \
        rng.normal(size=(ntri, 3, 3)) * size[:, None, None]
    verts = np.ascontiguousarray(tris.reshape(-1, 3), np.float32)
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    v = verts.reshape(-1, 3, 3).astype(np.float64)
    kind = rng.choice(np.array([3, 4]), N, p=[0.7, 0.3])
    k = rng.integers(0, ntri, N)
    b = np.eye(3)[rng.integers(0, 3, N)]  # a vertex; an edge: one barycentric 0
    edge = np.flatnonzero(kind == 3)
    pair = rng.dirichlet([1, 1], edge.size)
    zero = rng.integers(0, 3, edge.size)
    for j in range(3):
        sel = zero == j
        b[edge[sel]] = np.insert(pair[sel], j, 0.0, axis=1)
    Q = (v[k] * b[:, :, None]).sum(1)
    P = L + (Q - L) * rng.uniform(1.01, 3.0, N)[:, None]
    d = P - CAM_POS
    t = np.linalg.norm(d, axis=1)
    flags = rng.choice(np.array([0, 1, 7], np.int32), N, p=[0.8, 0.1, 0.1])
    return types.SimpleNamespace(case="C", W=W, H=H, lg=lg, N=N, C=lg[0] * lg[1], lcam=lcam, verts=verts, faces=faces,
                                 F=len(faces), kind=kind, k=k, t=t.astype(np.float32), flags=flags,
                                 dirs=np.ascontiguousarray((d / t[:, None]).astype(np.float32).reshape(-1)),
                                 cam_pos=CAM_POS.astype(np.float32))


def launch_blocks(S):
    return (S.W // 8) * (S.H // 8)


def band_of(S, rows):
    lo, hi = rows if rows is not None else (0, S.H // 8)
    return lo * 8 * S.W, (hi - lo) * 8 * S.W


@functools.lru_cache(maxsize=None)
def light_grid(O, case, slabs=1, xM=PI_F):
    S = synthetic(O, case)
    return O.grid_spherical(S.lcam.cc, S.faces, S.verts, S.lg[0], S.lg[1], xM=xM, yM=xM, slabs=slabs)


def traced_pixels(S, st, strict):
    """The pixels of the rays the launch traces: chunks [0, min(nchunks, blocks) - 1) under the strict rule."""
    n, nch = st["n"], st["nchunks"]
    kend = max(min(nch, launch_blocks(S)) - 1, 0) if strict else nch
    M = int(st["prefix"][kend]) if kend < nch else n
    mask = np.zeros(S.N, bool)
    mask[st["map"][:M]] = True
    return mask


def shadow_stage(O, S, strict, rows=None, slabs=1, xM=PI_F, t=None, dirs=None, grid=None, cells=None):
    """The oracle's stage on the inputs of S (or on t, dirs, a light grid or ray cells put in their place)."""
    p0, n = band_of(S, rows)
    t = S.t if t is None else t
    dirs = S.dirs if dirs is None else dirs
    grid = light_grid(O, S.case, slabs, xM) if grid is None else grid
    m = O.map_rays(S.lcam.cc, t, dirs, S.cam_pos, S.lg[0], S.lg[1], p0, n, xM=xM, yM=xM)
    if cells is not None:
        m[n:] = cells
    st = dict(map_unsorted=m.copy(), n=n, p0=p0)
    cap = n // 64 + S.C + 2
    prefix, nch = O.process_rays(m, n, S.C + 1, cap)
    flags = S.flags.copy()
    O.trace_shadow(S.lcam.cc, grid, S.C, S.verts, S.faces, t, dirs, flags, m, prefix, S.cam_pos, nch, launch_blocks(S),
                   n, strict=strict, slabs=slabs)
    st.update(map=m, prefix=prefix, nchunks=nch, flags=flags, cap=cap)
    st["traced"] = traced_pixels(S, st, strict)
    return st


@functools.lru_cache(maxsize=None)
def want(O, case, strict, rows=None, slabs=1, xM=PI_F):
    return shadow_stage(O, synthetic(O, case), strict, rows, slabs, xM)


def cell_of_pixel(S, st):
    cells = np.full(S.N, -1, np.int64)
    cells[st["map_unsorted"][:st["n"]]] = st["map_unsorted"][st["n"]:]
    return cells


def in_own_list(S, g, cells):
    """Per pixel: triangle k of the ray is in the list of the ray's own cell."""
    out = np.zeros(S.N, bool)
    for p in np.flatnonzero((cells >= 0) & (cells < S.C)):
        c = cells[p]
        out[p] = (g["vals"][g["offset"][c]:g["offset"][c] + g["span"][c]] == S.k[p]).any()
    return out


# ------------------------------------------------------------------------------------------------ CPU: the inputs

@pytest.mark.parametrize("case", sorted(CASES))
def test_inputs_can_fail(O, case):
    """Conditions on the oracle alone that make the GPU comparisons of the case worth running."""
    S, g = synthetic(O, case), light_grid(O, case)
    lx, ly = S.lg
    every, strict = want(O, case, False), want(O, case, True)
    used = np.flatnonzero(g["span"])
    cells = cell_of_pixel(S, every)
    real = cells[(cells >= 0) & (cells < S.C)]
    per_cell = np.bincount(real, minlength=S.C)
    print("%s: %d triangles, R %d, cells used %d of %d, rows %d, columns %d, longest list %d; ray cells %d in %d rows, most "
          "rays in a cell %d, chunks %d against %d blocks" % (
              case, S.F, g["R"], used.size, S.C, np.unique(used % ly).size, np.unique(used // ly).size, g["span"].max(),
              (per_cell > 0).sum(), np.unique(real % ly).size, per_cell.max(), every["nchunks"], launch_blocks(S)))
    # the light grid
    assert np.unique(used % ly).size == ly and np.unique(used // ly).size >= 0.9 * lx
    assert len(set(S.list_cells)) == len(LIST_LENGTHS) and not set(S.list_cells) & set(S.stack_cells)
    assert [int(g["span"][c]) for c in S.list_cells] == list(LIST_LENGTHS)
    assert g["span"][S.stack_cells].min() >= (XSEG_LAST + 1) * 64 + 1 and (S.stack_cells >= 0).all()
    wide_spans = np.sort(g["sizes"][:S.first_stack])[::-1]
    assert (wide_spans >= 16).sum() >= 5, wide_spans[:8]  # a handful of triangles span many cells
    # the rays
    assert np.unique(real % ly).size == ly and (per_cell > 0).sum() >= 200
    assert per_cell.max() > 8192  # more than one beam at the largest "shadow_beam"
    assert ((per_cell >= 1) & (per_cell <= 64)).sum() >= 8
    assert (per_cell[S.list_cells] > 0).all()  # the lists of 1, 63, 64, 65, 129 are walked
    if case == "A":
        assert every["nchunks"] > launch_blocks(S)  # the strict launch rule cuts
        assert strict["traced"].sum() < every["traced"].sum() == S.N
    fresh = S.flags != 1  # (an incoming 1 says nothing about the trace)
    for st in (strict, every):
        sel = st["traced"] & fresh & (cells < S.C)
        out = st["flags"][sel]
        print("  %s: traced %d, shadowed %d, lit %d" % ("strict" if st is strict else "all chunks", st["traced"].sum(),
                                                        (out == 1).sum(), (out != 1).sum()))
        assert (out == 1).sum() >= 1000 and (out != 1).sum() >= 1000
        # the pass only ever writes 1
        assert ((st["flags"] == S.flags) | (st["flags"] == 1)).all()
        assert (st["flags"][~st["traced"]] == S.flags[~st["traced"]]).all()
        assert set(np.unique(st["flags"][S.flags == 7])) == {1, 7} and (st["flags"][S.flags == 1] == 1).all()
    sel = every["traced"] & fresh
    out = every["flags"]
    edge = sel & ((S.kind == 3) | (S.kind == 4))
    print("  edge and vertex rays: shadowed %d, lit %d" % ((out[edge] == 1).sum(), (out[edge] != 1).sum()))
    assert (out[edge] == 1).sum() >= 100 and (out[edge] != 1).sum() >= 100
    for j, off in enumerate(EPS_OFFSETS):
        o = out[sel & (S.kind == 5) & (S.offset == j)]
        print("  occluder distance + %g: shadowed %d, lit %d" % (off, (o == 1).sum(), (o != 1).sum()))
        assert (o == 1).any() and (o != 1).any(), off
    assert (out[sel & (S.kind == 10)] != 1).sum() >= 64
    assert (cells[S.kind == 10] == S.stack_cells[0]).sum() >= 64
    # rays built to be shadowed are: the occluder is in the ray's own list, the ray is traced
    built = sel & (S.kind == 1) & in_own_list(S, g, cells)
    print("  kind 1 with k in the ray's list: %d, flagged %d" % (built.sum(), (out[built] == 1).sum()))
    assert built.sum() >= 1000 and (out[built] == 1).all()
    for k in (7, 8, 9):
        assert (S.kind == k).sum() >= 64
    assert np.isnan(S.t).sum() == 0 and np.isnan(S.dirs).sum() == 0  # (the NaN is the stage's own: 0/0 at P == L)


@pytest.mark.parametrize("case", sorted(CASES))
def test_broken_stages_change_the_flags(O, case):
    """What a pass would compute that cut the lists short, lost the rows, or moved the edge rays a little."""
    S, g = synthetic(O, case), light_grid(O, case)
    every = want(O, case, False)
    base = every["flags"]
    np.testing.assert_array_equal(shadow_stage(O, S, False)["flags"], base)  # the rerun is the case's
    cut = dict(g, span=np.minimum(g["span"], 64).astype(np.uint32))
    changed = (shadow_stage(O, S, False, grid=cut)["flags"] != base).sum()
    print("%s: lists cut at 64 entries: %d flags change" % (case, changed))
    assert changed >= 100
    cells = every["map_unsorted"][S.N:].astype(np.int64)
    real = cells < S.C
    common = np.bincount(cells[real] % S.lg[1]).argmax()
    forced = np.where(real, cells // S.lg[1] * S.lg[1] + common, cells).astype(np.uint32)
    changed = (shadow_stage(O, S, False, cells=forced)["flags"] != base).sum()
    print("%s: every row forced to row %d: %d flags change" % (case, common, changed))
    assert changed >= 100
    rng = np.random.default_rng(5)
    dirs = S.dirs.astype(np.float64).reshape(-1, 3).copy()
    sel = (S.kind == 3) | (S.kind == 4)
    dirs[sel] *= 1.0 + 1e-4 * rng.normal(size=(int(sel.sum()), 3))
    moved = shadow_stage(O, S, False, dirs=np.ascontiguousarray(dirs.astype(np.float32).reshape(-1)))
    changed = (moved["flags"] != base)[sel].sum()
    print("%s: edge and vertex rays moved by 1e-4: %d flags change" % (case, changed))
    assert changed >= 100


MARGIN_MOVES = (1e-6, 1e-5)  # relative: the scale of the beam cull's margins (6/65536 of the operands, 1e-6 on a box)


def lone_rays(O):
    """Case C: per pixel, the ray is alone in its light cell, which holds its triangle k; its incoming flag is not 1."""
    S, g, every = synthetic(O, "C"), light_grid(O, "C"), want(O, "C", False)
    cells = cell_of_pixel(S, every)
    per_cell = np.bincount(cells[cells < S.C], minlength=S.C + 1)
    return (cells < S.C) & (per_cell[cells] == 1) & in_own_list(S, g, cells) & (S.flags != 1)


def test_sparse_case_is_sharp(O):
    """Case C puts the beam cull where a margin that is too small shows: at least 1000 edge and vertex rays are the only
    ray of their light cell, so the beam's box is the ray itself, with the triangle whose edge they pass in that cell's
    list; both outcomes occur at least 300 times among them; and at least 300 of their flags change when the rays move
    by 1e-6 and by 1e-5 of their direction, so the exact test decides them at the scale of the cull's margins."""
    S, every = synthetic(O, "C"), want(O, "C", False)
    assert set(np.unique(S.kind)) == {3, 4} and every["traced"].all()
    lone = lone_rays(O)
    out = every["flags"]
    print("C: %d triangles, R %d, %d chunks, lone edge and vertex rays %d: shadowed %d, lit %d" % (
        S.F, light_grid(O, "C")["R"], every["nchunks"], lone.sum(), (out[lone] == 1).sum(), (out[lone] != 1).sum()))
    assert lone.sum() >= 1000 and (out[lone] == 1).sum() >= 300 and (out[lone] != 1).sum() >= 300
    cells = cell_of_pixel(S, every)
    for rel in MARGIN_MOVES:
        rng = np.random.default_rng(7)
        dirs = S.dirs.astype(np.float64).reshape(-1, 3) * (1.0 + rel * rng.normal(size=(S.N, 3)))
        moved = shadow_stage(O, S, False, dirs=np.ascontiguousarray(dirs.astype(np.float32).reshape(-1)))
        changed = lone & (moved["flags"] != out) & (cell_of_pixel(S, moved) == cells)  # (still in the same list)
        print("C: lone rays moved by %g: %d flags change" % (rel, changed.sum()))
        assert changed.sum() >= 300
    strict = want(O, "C", True)
    assert 0 < strict["traced"].sum() < S.N and strict["nchunks"] > launch_blocks(S)


def test_half_extent_sends_rays_to_the_sentinel_cell(O):
    S = synthetic(O, "A")
    cells = want(O, "A", False, xM=HALF_PI_F)["map_unsorted"][S.N:]
    assert (cells == S.C).sum() >= 1000 and (cells < S.C).sum() >= 1000 and (cells <= S.C).all()


def test_band_rays_differ_from_the_frame_s(O):
    S = synthetic(O, "A")
    st = want(O, "A", False, rows=BAND_ROWS)
    p0, n = band_of(S, BAND_ROWS)
    assert (p0, n) == (8192, 16384) and st["traced"].sum() == n
    assert st["traced"][p0:p0 + n].all() and (st["flags"] != S.flags).sum() >= 1000


# ------------------------------------------------------------------------------------------------ the reference's kernels

REF_STAGES = ("sph", "map", "chunks", "shadow")
RECORD = "shadowsyn"


def ref_stage_inputs(O):
    """Case A as the reference's kernels take it (oracle/ref_kernels.cpp), strict chunks, every input the oracle's."""
    S, g, st = synthetic(O, "A"), light_grid(O, "A"), want(O, "A", True)
    verts, faces = S.verts.reshape(-1), S.faces.reshape(-1)
    n = st["nchunks"]
    return {
        "sph": dict(cc=S.lcam.cc, faces=faces, verts=verts, nbx=S.lg[0], nby=S.lg[1], xM=PI_F, yM=PI_F, scan=g["scan"]),
        "map": dict(cc=S.lcam.cc, t=S.t, dir=S.dirs, cam_pos=S.cam_pos, W=S.W, H=S.H, xM=PI_F, yM=PI_F),
        "chunks": dict(d_map=st["map"], W=S.W, H=S.H),
        "shadow": dict(cc=S.lcam.cc, vals=g["vals"], span=g["span"], offset=g["offset"], verts=verts, faces=faces, t=S.t,
                       dir=S.dirs, is_shadowed=S.flags, d_map=st["map"], prefix=st["prefix"][:n], cam_pos=S.cam_pos,
                       nchunks=n, W=S.W, H=S.H),
    }


def nan_angle(S):
    """(x, y): the rays whose column, whose row angle is acos(0/0), by construction: P == L, and P on +-up (the
    column's projection has length 0) or on +-right (the row's)."""
    return (S.kind == 8) | np.isin(S.axis, (1, 4)), (S.kind == 8) | np.isin(S.axis, (2, 5))


def pinned(O, stage, out):
    """What of a stage's outputs is compared with the reference's kernels.  They are compiled for the host here, where
    the (int) of a NaN angle in getEffective_x/y is INT_MIN, or whatever else the host's conversion leaves; on the GPU
    it is 0, which is what the oracle and the product compute.  So the map's entries of the rays
    with such an angle are left out; test_nan_angles_map_as_on_the_gpu says what they are."""
    if stage != "map":
        return out
    S = synthetic(O, "A")
    keep = ~(nan_angle(S)[0] | nan_angle(S)[1])
    m = np.ascontiguousarray(out["d_map"])
    assert (m[:S.N] == np.arange(S.N)).all()
    return dict(out, d_map=np.concatenate([m[:S.N][keep], m[S.N:][keep]]))


def ref_oracle_outputs(O):
    S, g, st = synthetic(O, "A"), light_grid(O, "A"), want(O, "A", True)
    keys, vals = O.fill_2d(g["rng"], g["scan"], S.lg[1])
    n = st["nchunks"]
    return {"sph": dict(sizes=g["sizes"], zmin=g["zmin"], keys=keys, vals=vals), "map": dict(d_map=st["map_unsorted"]),
            "chunks": dict(prefix=st["prefix"][:n], nchunks=np.int32([n])), "shadow": dict(is_shadowed=st["flags"])}


def test_oracle_equals_reference_kernels_on_case_A(O):
    """The record of the reference's kernels on case A against the oracle, always; the live kernels where built."""
    import test_reference_kernels as RK

    rec = RK.load_record(RECORD)
    ins, outs = ref_stage_inputs(O), ref_oracle_outputs(O)
    for stage in REF_STAGES:
        assert RK.input_sha(ins[stage]) == str(rec[stage + "/input_sha"]), \
            "%s: stage inputs differ from the recorded ones (generator or oracle drift)" % stage
        RK.assert_matches_record(rec, RECORD, stage, pinned(O, stage, outs[stage]), "oracle")
    # the reference's run met a NaN angle once per ray on +-up or +-right and twice per ray at L, and nowhere else
    S = synthetic(O, "A")
    x, y = nan_angle(S)
    assert ((x & y) == (S.kind == 8)).all()
    assert int(rec["map/report/acos_nan"]) == (x ^ y).sum() + 2 * (x & y).sum() == x.sum() + y.sum()
    if O.ref_kernels_live():
        for stage in REF_STAGES:
            got = O.run_ref_kernels(stage, **ins[stage])
            RK.assert_matches_record(rec, RECORD, stage, pinned(O, stage, got), "reference")
            if stage == "map":
                assert int(got["acos_nan"][0]) == int(rec["map/report/acos_nan"])
                # which rays they are: the host's (int) of a NaN column is INT_MIN, so exactly the rays of x land in
                # the sentinel cell here where the oracle has a real one, and no ray outside x | y differs at all
                m, mine = np.ascontiguousarray(got["d_map"]), outs["map"]["d_map"]
                differs = m[S.N:] != mine[S.N:]
                assert (differs == x).all() and (m[S.N:][x] == S.C).all() and (mine[S.N:][x] < S.C).all()


@pytest.mark.parametrize("case", sorted(CASES))
def test_nan_angles_map_as_on_the_gpu(O, case):
    """A NaN angle converts to 0 (ugrt_f2i / ugrt_f2u, as CUDA and CDNA convert): the column is the middle one, the row
    is row 0; such a ray lies in a real cell and is traced."""
    S = synthetic(O, case)
    cells = cell_of_pixel(S, want(O, case, False))
    x, y = nan_angle(S)
    assert x.sum() >= 64 and y.sum() >= 64 and (x & ~y).sum() >= 8 and (y & ~x).sum() >= 8
    assert (cells[x] // S.lg[1] == S.lg[0] // 2).all() and (cells[y] % S.lg[1] == 0).all()
    assert (cells[S.kind == 8] == S.lg[0] // 2 * S.lg[1]).all()


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def u32(t):
    return t.cpu().numpy().view(np.uint32)


class Stage:
    """A context with the light camera uploaded as use_light_camera does, and the case's arrays on the device."""

    def __init__(self, ugrt, S, flags=0, rows=None, slabs=1):
        self.u, self.S = ugrt, S
        self.ctx = ctx = ugrt.Context(S.W, S.H, light_grid=S.lg, rows=rows, flags=flags, slabs=slabs)
        cam = ugrt.renderer.make_camera(LIGHT, FOVY, aspect_of(S.W, S.H))
        np.testing.assert_array_equal(bits(cam.camcoords), bits(S.lcam.cc))
        ugrt.renderer.use_light_camera(ctx, cam)
        self.verts, self.faces = ctx.upload(S.verts.reshape(-1)), ctx.upload(S.faces.reshape(-1))
        self.t, self.dirs, self.cam_pos = ctx.upload(S.t), ctx.upload(S.dirs), ctx.upload(S.cam_pos)
        self.n, self.cap = ctx.npix, ctx.prefix_capacity()
        self.build()

    def sentinel(self, n):
        return self.ctx.upload(np.full(n, SENT, np.uint32).view(np.int32))

    def build(self, xM=PI_F):
        self.ctx.grid_build_spherical(self.faces, self.verts, self.S.F, xM, xM)

    def map(self, xM=PI_F):
        buf = self.sentinel(2 * self.n + TAIL)
        self.ctx.map_rays_to_light(self.t, self.dirs, buf, self.cam_pos, xM, xM)
        return buf

    def sort(self, buf, deferred=False):
        prefix = self.sentinel(self.cap + TAIL)
        return prefix, self.ctx.sort_rays(buf, prefix[:self.cap], deferred=deferred)

    def trace(self, buf, prefix, count, flags=None):
        lvalue, lspan, loffset, _ = self.ctx.grid_ptrs(self.u.GRID_SPHERICAL)
        flags = self.ctx.upload(self.S.flags.copy()) if flags is None else flags
        self.ctx.trace_shadow(lvalue, self.verts, self.faces, lspan, loffset, self.t, self.dirs, flags, buf, prefix,
                              self.cam_pos, count)
        self.ctx.synchronize()
        return flags

    def run(self, deferred=False):
        """map, sort, trace: (map buffer, prefix buffer, count as the sort returned it, flags)."""
        buf = self.map()
        prefix, count = self.sort(buf, deferred)
        return buf, prefix, count, self.trace(buf, prefix, count).cpu().numpy()


@pytest.fixture(scope="module")
def stage(ugrt, O, torch):
    """stage(case, all_chunks, rows, slabs): one context per form of a case, with its light grid built, shared by the
    tests of this file (each maps, sorts and traces into buffers of its own) and dropped behind the last of them."""
    made = {}

    def get(case, all_chunks=False, rows=None, slabs=1):
        key = (case, all_chunks, rows, slabs)
        if key not in made:
            made[key] = Stage(ugrt, synthetic(O, case), ugrt.FLAG_SHADOW_ALL_CHUNKS if all_chunks else 0, rows, slabs)
        return made[key]

    yield get
    made.clear()


def assert_map_equal(got, unsorted_or_sorted, n, what):
    got = u32(got)
    assert got.size == 2 * n + TAIL
    bad = np.flatnonzero(got[:2 * n] != unsorted_or_sorted)
    assert bad.size == 0, "%s: %d of %d map words differ, first at %d: %d, oracle %d" % (
        what, bad.size, 2 * n, bad[0], got[bad[0]], unsorted_or_sorted[bad[0]])
    assert (got[2 * n:] == SENT).all(), what + ": written behind the map"


def assert_sorted_equal(s, buf, prefix, count, w, what):
    assert count == w["nchunks"], (what, count, w["nchunks"])
    assert_map_equal(buf, w["map"], s.n, what + ": sorted map")
    got = u32(prefix)
    np.testing.assert_array_equal(got[:count], w["prefix"][:count], err_msg=what + ": chunk starts")
    assert (got[s.cap:] == SENT).all(), what + ": written behind the chunk starts"


def assert_flags_equal(got, w, what):
    bad = np.flatnonzero(got != w["flags"])
    assert bad.size == 0, "%s: %d flags differ, first at pixel %d: %d, oracle %d" % (
        what, bad.size, bad[0], got[bad[0]], w["flags"][bad[0]])


def assert_grid_equal(ugrt, ctx, g, what):
    value, key, span, offset, gi = ctx.grid_arrays(ugrt.GRID_SPHERICAL)
    assert (gi.total_refs, gi.num_cells, gi.cells_used) == (g["R"], len(g["span"]), g["used"]), what
    for name, got, w in (("keys", key, g["keys"]), ("values", value, g["vals"]), ("span", span, g["span"]),
                         ("offset", offset, g["offset"])):
        np.testing.assert_array_equal(u32(got), w, err_msg="%s: %s" % (what, name))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES) + ["C"])
def test_light_grid(ugrt, O, stage, case):
    s = stage(case)
    for rep in range(2):
        s.build()
        s.ctx.synchronize()
        assert_grid_equal(ugrt, s.ctx, light_grid(O, case), "%s build %d" % (case, rep))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES) + ["C"])
def test_map(ugrt, O, stage, case):
    """Word for word, NaN, pole and t <= 0 rays included; nothing is written behind the 2n entries."""
    s = stage(case)
    for xM in (PI_F, HALF_PI_F):
        assert_map_equal(s.map(xM), want(O, case, False, xM=xM)["map_unsorted"], s.n, "%s extent %g" % (case, xM))


@pytest.mark.gpu
def test_map_of_a_band(ugrt, O, stage):
    s = stage("A", rows=BAND_ROWS)
    assert (s.ctx.p0, s.n) == band_of(s.S, BAND_ROWS)
    assert_map_equal(s.map(), want(O, "A", False, rows=BAND_ROWS)["map_unsorted"], s.n, "band")


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES) + ["C"])
def test_sort(ugrt, O, stage, case):
    s = stage(case)
    buf = s.map()
    prefix, count = s.sort(buf)
    assert_sorted_equal(s, buf, prefix, count, want(O, case, True), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES) + ["C"])
def test_trace_strict(ugrt, O, stage, case):
    """The reference's launch rule, with the count read back and with the count left on the device; twice on one
    context: the pass's state is re-armed.  Untraced pixels keep their incoming 0, 1 or 7."""
    s, w = stage(case), want(O, case, True)
    for rep, deferred in enumerate((False, True, False)):
        buf, prefix, count, flags = s.run(deferred)
        what = "%s call %d%s" % (case, rep, ", deferred" if deferred else "")
        assert count == (ugrt.CHUNKS_ON_DEVICE if deferred else w["nchunks"]), what
        assert_flags_equal(flags, w, what)
        assert_sorted_equal(s, buf, prefix, s.ctx.sort_rays_chunks(), w, what)


@pytest.mark.gpu
def test_trace_all_chunks(ugrt, O, stage):
    s, w = stage("A", all_chunks=True), want(O, "A", False)
    buf, prefix, count, flags = s.run()
    assert_flags_equal(flags, w, "waiting sort")
    assert_sorted_equal(s, buf, prefix, count, w, "waiting sort")
    # the deferred sort is put off: the trace reads the unsorted map, and processData's outputs come when asked for
    buf, prefix, count, flags = s.run(deferred=True)
    assert count == ugrt.CHUNKS_ON_DEVICE
    assert_flags_equal(flags, w, "deferred sort")
    assert_map_equal(buf, w["map_unsorted"], s.n, "deferred sort: the map behind the trace")
    assert_sorted_equal(s, buf, prefix, s.ctx.sort_rays_chunks(), w, "deferred sort, asked for")
    buf, prefix, count, flags = s.run()
    assert_flags_equal(flags, w, "waiting sort again")


@pytest.mark.gpu
@pytest.mark.parametrize("beam", [-1, 64, 8192], ids=["default beam", "shadow_beam64", "shadow_beam8192"])
def test_trace_of_lone_edge_rays(ugrt, O, stage, beam):
    """Case C, every chunk: a beam per ray, whose box is the ray (test_sparse_case_is_sharp)."""
    s, w = stage("C", all_chunks=True), want(O, "C", False)
    try:
        s.ctx.set_option("shadow_beam", beam)
        buf, prefix, count, flags = s.run()
    finally:
        s.ctx.set_option("shadow_beam", -1)
    assert_flags_equal(flags, w, "lone rays")
    assert_sorted_equal(s, buf, prefix, count, w, "lone rays")
    assert s.ctx.get_state("shadow_key_bits") == key_bits(s.S) == 32


@pytest.mark.gpu
@pytest.mark.parametrize("all_chunks", [False, True])
def test_trace_of_a_band(ugrt, O, stage, all_chunks):
    s, w = stage("A", all_chunks=all_chunks, rows=BAND_ROWS), want(O, "A", not all_chunks, rows=BAND_ROWS)
    buf, prefix, count, flags = s.run()
    assert_flags_equal(flags, w, "band")
    assert_sorted_equal(s, buf, prefix, count, w, "band")
    p0, n = band_of(s.S, BAND_ROWS)
    outside = np.ones(s.S.N, bool)
    outside[p0:p0 + n] = False
    np.testing.assert_array_equal(flags[outside], s.S.flags[outside])


@pytest.mark.gpu
@pytest.mark.parametrize("all_chunks", [False, True])
def test_trace_over_slabs(ugrt, O, stage, all_chunks):
    s, w = stage("B", all_chunks=all_chunks, slabs=3), want(O, "B", not all_chunks, slabs=3)
    g = light_grid(O, "B", slabs=3)
    assert len(g["span"]) == 3 * s.S.C and min(int(g["span"][q::3].sum()) for q in range(3)) > 0
    buf, prefix, count, flags = s.run()
    assert_grid_equal(ugrt, s.ctx, g, "slabs")
    assert_flags_equal(flags, w, "slabs")
    assert_sorted_equal(s, buf, prefix, count, w, "slabs")


def key_bits(S, key64=False, mbits=None):
    import test_light_grid_sizes as LG

    return LG.key_bits(S.lg, key64=key64, mbits=mbits)


# each set alone, then reset to -1: (options, key bits of the pass)
SHAPES = [((("shadow_beam", 64),), {}), ((("shadow_beam", 4096),), {}), ((("shadow_beam", 8192),), {}),
          ((("shadow_xseg", 64),), {}), ((("shadow_xseg", 1 << 20),), {}),
          ((("shadow_mbits", 1),), dict(mbits=1)), ((("shadow_mbits", 8),), dict(mbits=8)),
          ((("shadow_key64", 1),), dict(key64=True)),
          ((("shadow_sieve", 0),), {}), ((("shadow_sieve", 64),), {}),
          ((("shadow_xcd_run", 0), ("shadow_waves", 64)), {}),
          ((("shadow_itemsort", 0),), {}), ((("shadow_sizebits", 0),), {}),
          ((("sort_library", 1),), {}), ((("sort_items", 8), ("sort_rank", 0)), {})]


@pytest.mark.gpu
@pytest.mark.parametrize("options,key", SHAPES, ids=["-".join("%s%d" % o for o in opts) for opts, _ in SHAPES])
def test_launch_shapes_change_no_flag(ugrt, O, stage, options, key):
    s, w = stage("A", all_chunks=True), want(O, "A", False)
    try:
        for name, value in options:
            s.ctx.set_option(name, value)
        buf, prefix, count, flags = s.run()
        assert s.ctx.get_state("shadow_key_bits") == key_bits(s.S, **key)
    finally:
        for name, _ in options:
            s.ctx.set_option(name, -1)
    assert_flags_equal(flags, w, str(options))
    assert_sorted_equal(s, buf, prefix, count, w, str(options))
    buf, prefix, count, flags = s.run()  # ... and the defaults are back
    assert s.ctx.get_state("shadow_key_bits") == key_bits(s.S) == 32
    assert_flags_equal(flags, w, "after " + str(options))


@pytest.mark.gpu
def test_product_equals_reference_record(ugrt, O, stage):
    """Case A through libugrt.so against the record of the reference's kernels, no oracle in between: the unsorted map,
    the sorted one's chunk starts, and the flags under the reference's launch rule."""
    import test_reference_kernels as RK

    rec = RK.load_record(RECORD)
    s = stage("A")
    buf = s.map()
    RK.assert_matches_record(rec, RECORD, "map", pinned(O, "map", dict(d_map=u32(buf)[:2 * s.n])), "product")
    prefix, count = s.sort(buf)
    assert count == int(rec["chunks/nchunks"][0])
    RK.assert_matches_record(rec, RECORD, "chunks", dict(prefix=u32(prefix)[:count], nchunks=np.int32([count])), "product")
    RK.assert_matches_record(rec, RECORD, "shadow", dict(is_shadowed=s.trace(buf, prefix, count).cpu().numpy()), "product")
