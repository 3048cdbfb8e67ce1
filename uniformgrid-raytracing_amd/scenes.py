"""Procedural scenes for the BASELINE configs (no .obj ships with the reference).

Every generator writes a real Wavefront ``.obj`` + ``.mtl`` (so the loader path
is exercised) and the reference's positional material file
(``Model::some_material``, scene.h:370-439: per material 3 tokens, 3 floats Ka,
1 token, 3 floats Kd, 11 tokens, 1 texture token or ``NA``).  Seed 20100502
(SURVEY.md section 8d).  Coordinates are written with 6 decimals; both loaders
parse the same text, so the float32 vertex arrays are identical.

  cornell()  -- the public Cornell box data, 16 quads pre-triangulated = 32 tris
  hall()     -- "Sibenik"-class stand-in: room [0,28]x[0,26]x[0,9], 24 columns,
                stepped dais, vaulted ceiling; ~80 k tris, 6 materials
  crash()    -- "crashing"-class stand-in: the room + table + 20 chairs
                (200 000 tris) + icosphere level 7 (327 680) + debris shards
                = 1 000 000 tris; sphere + shards are the animated sub-range
  mirrors()  -- a corridor between two facing mirror walls over a reflective
                floor, boxes and an icosphere between them: reflections of
                many levels (Renderer.display(..., bounces=D))
  glass()    -- a small room with a glass icosphere, a glass slab in front of
                two boxes and a mirror panel: rays that go through solids
                (Renderer.display(..., reflect=True, refract=True))
  glossy()   -- a room whose reflecting floor is split into three strips of
                sharpness 1000, 700 and 300 under rows of thin coloured posts
                and a column: rough mirrors (Renderer.display(..., glossy=S))
  depth()    -- a floor with five identical thin posts at growing distances
                along the view: a lens focused on the middle one
                (Renderer.display(..., dof=S, dof_aperture=a))
"""
import os

import numpy as np

SEED = 20100502

# main.cu:87-90, :158-164, per_frame_funcs.h:8-10
REF_CAMERA = dict(eye=(3, 15, 5), look=(13, 13, 3), up=(0, 0, 1), near=0.1, far=100.0)
REF_LIGHT_CAMERA = dict(eye=(14, 13, 8), look=(14, 13, 0.0), up=(0, 1, 0), near=0.1, far=100.0)
REF_SHADING_LIGHT = (10.0, 12.0, 6.0)


class Mesh:
    def __init__(self):
        self.v, self.f, self.m = [], [], []
        self.nv = 0

    def add(self, verts, faces, mat):
        verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
        faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        self.v.append(verts)
        self.f.append(faces + self.nv)
        self.m.append(np.full(len(faces), mat, dtype=np.int32))
        self.nv += len(verts)

    def ntris(self):
        return int(sum(len(f) for f in self.f))

    def arrays(self):
        return (np.concatenate(self.v), np.concatenate(self.f).astype(np.int32), np.concatenate(self.m))


def grid_quad(p0, du, dv, nu, nv):
    """Tessellated parallelogram p0 + s*du + t*dv, nu x nv quads -> 2*nu*nv triangles."""
    p0, du, dv = (np.asarray(a, dtype=np.float64) for a in (p0, du, dv))
    s = np.linspace(0.0, 1.0, nu + 1)
    t = np.linspace(0.0, 1.0, nv + 1)
    S, T = np.meshgrid(s, t, indexing="ij")
    verts = p0 + S[..., None] * du + T[..., None] * dv
    idx = np.arange((nu + 1) * (nv + 1)).reshape(nu + 1, nv + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return verts.reshape(-1, 3), faces


def add_box(mesh, lo, hi, n, mat, faces="xyzXYZ"):
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    d = hi - lo
    ex, ey, ez = np.array([d[0], 0, 0]), np.array([0, d[1], 0]), np.array([0, 0, d[2]])
    quads = {
        "x": (lo, ey, ez), "X": (lo + ex, ey, ez), "y": (lo, ex, ez), "Y": (lo + ey, ex, ez),
        "z": (lo, ex, ey), "Z": (lo + ez, ex, ey),
    }
    for k in faces:
        mesh.add(*grid_quad(*quads[k], n, n), mat)


def add_cylinder(mesh, cx, cy, z0, z1, r, nseg, nstack, mat, flutes=0):
    th = np.linspace(0.0, 2 * np.pi, nseg + 1)
    z = np.linspace(z0, z1, nstack + 1)
    TH, Z = np.meshgrid(th, z, indexing="ij")
    rr = r * (1.0 + (0.06 * np.cos(flutes * TH) if flutes else 0.0))
    verts = np.stack([cx + rr * np.cos(TH), cy + rr * np.sin(TH), Z], -1)
    idx = np.arange((nseg + 1) * (nstack + 1)).reshape(nseg + 1, nstack + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    mesh.add(verts.reshape(-1, 3), faces, mat)


def add_vault(mesh, x0, x1, y0, y1, zbase, rise, nu, nv, mat):
    """Barrel vault along x over [y0,y1]."""
    s = np.linspace(0.0, 1.0, nu + 1)
    t = np.linspace(0.0, np.pi, nv + 1)
    S, T = np.meshgrid(s, t, indexing="ij")
    verts = np.stack([x0 + S * (x1 - x0), (y0 + y1) / 2 - np.cos(T) * (y1 - y0) / 2, zbase + rise * np.sin(T)], -1)
    idx = np.arange((nu + 1) * (nv + 1)).reshape(nu + 1, nv + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    mesh.add(verts.reshape(-1, 3), faces, mat)


def icosphere(level):
    t = (1.0 + 5 ** 0.5) / 2
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5],
                  [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int64)
    for _ in range(level):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        e.sort(axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[ue[:, 0]] + v[ue[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        base = len(v)
        v = np.concatenate([v, mid])
        n = len(f)
        ab, bc, ca = base + inv[:n], base + inv[n:2 * n], base + inv[2 * n:]
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1),
                            np.stack([ab, bc, ca], 1)])
    return v, f


def add_room(mesh, n=40):
    """Room [0,28]x[0,26]x[0,9], walls tessellated n x n.  Materials: 0 floor, 1 walls, 2 ceiling.

    The wall x = 0 (behind the reference camera at (3,15,5)) is left out, like a stage set: the
    reference's primary intersection takes |t| (trace_kernel.cu:35), so a wall
    BEHIND the eye would win every pixel as a ghost hit and hide the scene.
    """
    add_box(mesh, (0, 0, 0), (28, 26, 9), n, 1, faces="XyY")
    add_box(mesh, (0, 0, 0), (28, 26, 9), n, 0, faces="z")
    add_box(mesh, (0, 0, 0), (28, 26, 9), n, 2, faces="Z")


MATERIALS_ROOM = [
    # name, Ka, Kd, reflect
    ("m0_floor", (0.2, 0.2, 0.2), (0.62, 0.58, 0.52), 0.5),
    ("m1_wall", (0.2, 0.2, 0.2), (0.80, 0.78, 0.70), 0.0),
    ("m2_ceiling", (0.2, 0.2, 0.2), (0.85, 0.85, 0.88), 0.0),
    ("m3_column", (0.2, 0.2, 0.2), (0.70, 0.66, 0.60), 0.0),
    ("m4_wood", (0.2, 0.2, 0.2), (0.55, 0.35, 0.20), 0.5),
    ("m5_object", (0.2, 0.2, 0.2), (0.80, 0.25, 0.20), 0.0),
]

MATERIALS_CORNELL = [
    ("c0_white", (0.2, 0.2, 0.2), (0.76, 0.75, 0.50), 0.0),
    ("c1_light", (0.2, 0.2, 0.2), (1.00, 1.00, 1.00), 0.0),
    ("c2_green", (0.2, 0.2, 0.2), (0.15, 0.48, 0.09), 0.0),
    ("c3_red", (0.2, 0.2, 0.2), (0.63, 0.06, 0.04), 0.0),
]

CORNELL_QUADS = [
    # (material, 4 vertices)  -- the public Cornell box data
    (0, [(552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2)]),                 # floor
    (1, [(343, 548.8, 227), (343, 548.8, 332), (213, 548.8, 332), (213, 548.8, 227)]),  # light
    (0, [(556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0)]),      # ceiling
    (0, [(549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2)]),    # back wall
    (2, [(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)]),                  # right wall
    (3, [(552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0)]),      # left wall
    (0, [(130, 165, 65), (82, 165, 225), (240, 165, 272), (290, 165, 114)]),            # short block
    (0, [(290, 0, 114), (290, 165, 114), (240, 165, 272), (240, 0, 272)]),
    (0, [(130, 0, 65), (130, 165, 65), (290, 165, 114), (290, 0, 114)]),
    (0, [(82, 0, 225), (82, 165, 225), (130, 165, 65), (130, 0, 65)]),
    (0, [(240, 0, 272), (240, 165, 272), (82, 165, 225), (82, 0, 225)]),
    (0, [(423, 330, 247), (265, 330, 296), (314, 330, 456), (472, 330, 406)]),          # tall block
    (0, [(423, 0, 247), (423, 330, 247), (472, 330, 406), (472, 0, 406)]),
    (0, [(472, 0, 406), (472, 330, 406), (314, 330, 456), (314, 0, 456)]),
    (0, [(314, 0, 456), (314, 330, 456), (265, 330, 296), (265, 0, 296)]),
    (0, [(265, 0, 296), (265, 330, 296), (423, 330, 247), (423, 0, 247)]),
]


def write_scene(outdir, name, verts, faces, matidx, materials, glass=None, sharpness=None, uvs=None, uv_faces=None,
                textures=None):
    """Write <name>.obj, <name>.mtl, <name>.mat; returns their paths.  glass: {material index: (d, Ni)} -- the MTL
    carries these materials' dissolve and index of refraction, every other material is written as "d 1" without Ni.
    sharpness: {material index: value} -- the MTL carries these materials' "sharpness" line behind the dissolve, every
    other material has none (the loader's default is 98).
    uvs [T, 2] and uv_faces [F, 3] (indices into uvs, -1: none): the OBJ carries "vt" lines behind its vertices and the
    faces whose three corners have one are written as "f v/t v/t v/t".  textures: {material index: (file name, uint8 array
    [H, W, 3])} -- the MTL carries these materials' "map_Kd" line and the arrays are written as P6 files beside it.  With
    none of the three the files are what they were without these keywords, byte for byte."""
    os.makedirs(outdir, exist_ok=True)
    obj, mtl, mat = (os.path.join(outdir, name + e) for e in (".obj", ".mtl", ".mat"))
    with open(mtl, "w") as fp:
        for k, (nm, ka, kd, refl) in enumerate(materials):
            d_ni = "d 1\n" if not glass or k not in glass else "d %.6f\nNi %.6f\n" % tuple(glass[k])
            if sharpness and k in sharpness:
                d_ni += "sharpness %.6f\n" % sharpness[k]
            if textures and k in textures:
                d_ni += "map_Kd %s\n" % textures[k][0]
                tex = np.ascontiguousarray(textures[k][1], dtype=np.uint8)
                with open(os.path.join(outdir, textures[k][0]), "wb") as tp:
                    tp.write(b"P6\n%d %d\n255\n" % (tex.shape[1], tex.shape[0]) + tex.tobytes())
            fp.write("newmtl %s\nKa %.6f %.6f %.6f\nKd %.6f %.6f %.6f\nKs 1.000000 1.000000 1.000000\nNs 0\n"
                     "%sr %.6f\nillum 2\n\n" % ((nm,) + tuple(ka) + tuple(kd) + (d_ni, refl)))
    with open(mat, "w") as fp:
        for nm, ka, kd, refl in materials:
            fp.write("newmtl %s Ka %.6f %.6f %.6f Kd %.6f %.6f %.6f Ks 1 1 1 Ns 0 d 1 r %.6f map NA\n"
                     % ((nm,) + tuple(ka) + tuple(kd) + (refl,)))
    with open(obj, "w") as fp:
        fp.write("# generated by uniformgrid-raytracing_amd.scenes (seed %d)\nmtllib %s.mtl\n" % (SEED, name))
        fp.write("".join("v %.6f %.6f %.6f\n" % tuple(r) for r in verts))
        if uvs is not None:
            fp.write("".join("vt %.6f %.6f\n" % tuple(r) for r in np.asarray(uvs).reshape(-1, 2)))
        t1 = None if uvs is None or uv_faces is None else np.asarray(uv_faces).reshape(-1, 3) + 1
        # usemtl only when the material changes
        change = np.flatnonzero(np.diff(matidx, prepend=-999))
        bounds = list(change) + [len(faces)]
        f1 = faces + 1
        for a, b in zip(bounds[:-1], bounds[1:]):
            fp.write("usemtl %s\n" % materials[int(matidx[a])][0])
            if t1 is None:
                fp.write("".join("f %d %d %d\n" % tuple(r) for r in f1[a:b]))
            else:
                fp.write("".join("f %d/%d %d/%d %d/%d\n" % (r[0], t[0], r[1], t[1], r[2], t[2]) if t.min() > 0
                                 else "f %d %d %d\n" % tuple(r) for r, t in zip(f1[a:b], t1[a:b])))
    return obj, mtl, mat


def _finish(outdir, name, mesh, materials, extra):
    verts, faces, matidx = mesh.arrays()
    info = dict(name=name, num_faces=len(faces), num_vertices=len(verts), materials=materials)
    info.update(extra)
    if outdir is not None:
        info["obj"], info["mtl"], info["mat"] = write_scene(outdir, name, verts, faces, matidx, materials,
                                                            extra.get("glass"), extra.get("sharpness_of"), extra.get("uvs"),
                                                            extra.get("uv_faces"), extra.get("texture_files"))
    info["verts"] = verts.astype(np.float32)  # generation values; the loaders parse the 6-decimal text
    info["faces"] = faces
    info["matidx"] = matidx
    info["mat_list"] = np.array([list(ka) + list(kd) for _, ka, kd, _ in materials], dtype=np.float32)
    info["reflect"] = np.array([r for _, _, _, r in materials], dtype=np.float32)
    return info


def cornell(outdir=None):
    mesh = Mesh()
    for m, q in CORNELL_QUADS:
        mesh.add(q, [[0, 1, 2], [0, 2, 3]], m)
    mn, mx = np.array([0, 0, 0.0]), np.array([556, 548.8, 559.2])
    c = (mn + mx) / 2
    cams = {
        # main.cu:114-118 (the reference's commented Cornell camera) and a view from outside the box
        "A": dict(eye=tuple(c), look=(c[0], c[1], mx[2]), up=(0, 1, 0), near=1.0, far=650.0),
        "B": dict(eye=(278, 273, -800), look=(278, 273, 0), up=(0, 1, 0), near=1.0, far=2000.0),
    }
    light_cam = dict(eye=(278, 540, 279.5), look=(278, 0, 279.5), up=(0, 0, 1), near=1.0, far=2000.0)
    return _finish(outdir, "cornell", mesh, MATERIALS_CORNELL,
                   dict(cameras=cams, light_camera=light_cam, shading_light=(278.0, 500.0, 279.5)))


def _hall_static(mesh, wall_n=40, col_seg=32, col_stack=26, vault=(64, 160)):
    add_room(mesh, wall_n)
    k = 0
    for ix in range(12):
        for iy in range(2):  # two rows, the centre aisle stays open for the reference camera
            cx, cy = 3.0 + ix * 2.1, 5.0 + iy * 16.0
            add_cylinder(mesh, cx, cy, 0.0, 7.5, 0.45, col_seg, col_stack, 3, flutes=8)
            k += 1
    for s in range(3):
        add_box(mesh, (20 - s * 0.8, 8 + s * 0.8, s * 0.35), (27 + 0.0, 18 - s * 0.8, (s + 1) * 0.35), 10, 4,
                faces="xyYZX")
    add_vault(mesh, 0.5, 27.5, 1.0, 25.0, 7.5, 1.4, vault[0], vault[1], 2)


def hall(outdir=None, scale=1.0):
    """~80 000 triangles at scale 1 (scale < 1 shrinks the tessellation for CPU-sized tests)."""
    mesh = Mesh()
    s = max(0.05, scale) ** 0.5
    _hall_static(mesh, wall_n=max(2, int(40 * s)), col_seg=max(6, int(32 * s)), col_stack=max(2, int(26 * s)),
                 vault=(max(4, int(64 * s)), max(8, int(160 * s))))
    return _finish(outdir, "hall%dk" % round(mesh.ntris() / 1000), mesh, MATERIALS_ROOM,
                   dict(cameras={"ref": REF_CAMERA}, light_camera=REF_LIGHT_CAMERA,
                        shading_light=REF_SHADING_LIGHT))


def crash(outdir=None, scale=1.0):
    """1 000 000 triangles at scale 1: 200 000 static + icosphere(7) + shards (animated sub-range).

    The animated object lives in the reference's "orig" space (centre (12,11,4.5)),
    which copy_data_transform (transformation_kernel.cu:10-16) maps to (14.5,13,4).
    """
    rng = np.random.default_rng(SEED)
    mesh = Mesh()
    s = max(0.02, scale) ** 0.5
    add_room(mesh, max(2, int(40 * s)))
    n_box = max(1, int(12 * s))
    add_box(mesh, (10, 9, 1.4), (19, 17, 1.6), max(2, int(40 * s)), 4)  # table top
    for lx, ly in ((10.2, 9.2), (18.4, 9.2), (10.2, 16.4), (18.4, 16.4)):
        add_box(mesh, (lx, ly, 0), (lx + 0.4, ly + 0.4, 1.4), n_box, 4, faces="xXyY")
    for i in range(20):
        ang = 2 * np.pi * i / 20
        cx, cy = 14.5 + 7.0 * np.cos(ang), 13.0 + 6.0 * np.sin(ang)
        add_box(mesh, (cx - 0.35, cy - 0.35, 0.75), (cx + 0.35, cy + 0.35, 0.85), n_box, 4)
        add_box(mesh, (cx - 0.35, cy + 0.27, 0.85), (cx + 0.35, cy + 0.35, 1.8), n_box, 4)
        for dx, dy in ((-0.33, -0.33), (0.25, -0.33), (-0.33, 0.25), (0.25, 0.25)):
            add_box(mesh, (cx + dx, cy + dy, 0), (cx + dx + 0.08, cy + dy + 0.08, 0.75), max(1, n_box // 2), 4,
                    faces="xXyY")
    static_target = int(round(200000 * scale / 2)) * 2
    left = static_target - mesh.ntris()
    if left > 0:  # a rug that brings the static part to the exact count: near-square quads, not slivers
        q = left // 2
        nu = max(1, int((q * 11.0 / 9.0) ** 0.5))
        nv = max(1, q // nu)
        mesh.add(*grid_quad((9, 8.5, 0.01), (11, 0, 0), (0, 9, 0), nu, nv), 4)
        rest = q - nu * nv
        if rest > 0:  # fringe: `rest` small quads along one edge
            mesh.add(*grid_quad((9, 8.4, 0.01), (11.0 * rest / max(nu, rest), 0, 0), (0, 0.1, 0), rest, 1), 4)
    n_static_faces, n_static_verts = mesh.ntris(), mesh.nv
    level = 7 if scale >= 1.0 else max(1, int(round(7 + np.log(max(scale, 1e-3)) / np.log(4))))
    sv, sf = icosphere(level)
    mesh.add(sv * (2.0 * 12 / 9) + np.array([12, 11, 4.5]), sf, 5)
    total_target = int(round(1000000 * scale))
    nsh = max(0, total_target - mesh.ntris())
    if nsh:
        ctr = rng.normal(0.0, 2.0 * 12 / 9, size=(nsh, 3)) + np.array([12, 11, 4.5])
        ctr[:, 0] = np.clip(ctr[:, 0], 4.5, 19.5)
        ctr[:, 1] = np.clip(ctr[:, 1], 3.5, 18.5)
        ctr[:, 2] = np.clip(ctr[:, 2], 0.6, 8.4)
        edge = rng.uniform(0.02, 0.1, size=(nsh, 1, 1)) * 12 / 9
        tri = rng.normal(size=(nsh, 3, 3))
        tri /= np.linalg.norm(tri, axis=2, keepdims=True)
        verts = ctr[:, None, :] + tri * edge
        mesh.add(verts.reshape(-1, 3), np.arange(nsh * 3).reshape(-1, 3), 5)
    return _finish(outdir, "crash%dk" % round(mesh.ntris() / 1000), mesh, MATERIALS_ROOM,
                   dict(cameras={"ref": REF_CAMERA}, light_camera=REF_LIGHT_CAMERA,
                        shading_light=REF_SHADING_LIGHT, animated_offset=n_static_verts,
                        animated_size=mesh.nv - n_static_verts, static_faces=n_static_faces))


MATERIALS_MIRRORS = [
    # name, Ka, Kd, reflect
    ("r0_floor", (0.2, 0.2, 0.2), (0.55, 0.55, 0.60), 0.5),
    ("r1_mirror", (0.2, 0.2, 0.2), (0.70, 0.80, 0.90), 0.85),
    ("r2_end_wall", (0.2, 0.2, 0.2), (0.80, 0.78, 0.70), 0.0),
    ("r3_box", (0.2, 0.2, 0.2), (0.80, 0.25, 0.20), 0.0),
    ("r4_glossy_box", (0.2, 0.2, 0.2), (0.20, 0.45, 0.80), 0.3),
    ("r5_sphere", (0.2, 0.2, 0.2), (0.85, 0.75, 0.30), 0.6),
]


def mirrors(outdir=None, scale=1.0):
    """Corridor [0,30]x[0,4]x[0,4]: the long walls y = 0 and y = 4 are mirrors (reflect 0.85) facing each other, the
    floor reflects 0.5, the wall at x = 30 is matt; no ceiling and no wall at x = 0 (behind the camera: see add_room),
    so rays that climb leave the grid.  Between the mirrors: four boxes and an icosphere.  The camera looks obliquely
    down the corridor, so rays bounce from mirror to mirror many times.  ~40 000 triangles at scale 1."""
    mesh = Mesh()
    s = max(0.05, scale) ** 0.5
    n = max(2, int(48 * s))
    L, Wd, Hh = 30.0, 4.0, 4.0
    mesh.add(*grid_quad((0, 0, 0), (L, 0, 0), (0, Wd, 0), 2 * n, n // 2 + 1), 0)   # floor
    mesh.add(*grid_quad((0, 0, 0), (L, 0, 0), (0, 0, Hh), 2 * n, n // 2 + 1), 1)   # mirror y = 0
    mesh.add(*grid_quad((0, Wd, 0), (L, 0, 0), (0, 0, Hh), 2 * n, n // 2 + 1), 1)  # mirror y = Wd
    mesh.add(*grid_quad((L, 0, 0), (0, Wd, 0), (0, 0, Hh), n // 2 + 1, n // 2 + 1), 2)  # end wall
    nb = max(1, int(6 * s))
    for (x0, y0, sx, sy, h, m) in ((8.0, 0.8, 0.9, 0.9, 1.2, 3), (13.0, 2.4, 1.0, 0.8, 0.7, 4),
                                   (19.0, 1.2, 0.7, 1.2, 1.6, 3), (24.0, 2.6, 0.9, 0.9, 1.0, 4)):
        add_box(mesh, (x0, y0, 0.0), (x0 + sx, y0 + sy, h), nb, m, faces="xXyYZ")
    level = 4 if scale >= 1.0 else max(1, int(round(4 + np.log(max(scale, 1e-3)) / np.log(4))))
    sv, sf = icosphere(level)
    mesh.add(sv * 0.8 + np.array([16.0, 1.6, 1.6]), sf, 5)
    cams = {"ref": dict(eye=(1.0, 1.0, 1.7), look=(8.0, 3.6, 1.2), up=(0, 0, 1), near=0.1, far=100.0)}
    light_cam = dict(eye=(15.0, 2.0, 9.0), look=(15.0, 2.0, 0.0), up=(0, 1, 0), near=0.1, far=100.0)
    return _finish(outdir, "mirrors%dk" % round(mesh.ntris() / 1000), mesh, MATERIALS_MIRRORS,
                   dict(cameras=cams, light_camera=light_cam, shading_light=(15.0, 2.0, 3.5)))


MATERIALS_GLASS = [
    # name, Ka, Kd, reflect
    ("g0_floor", (0.2, 0.2, 0.2), (0.62, 0.60, 0.55), 0.0),
    ("g1_back_wall", (0.2, 0.2, 0.2), (0.30, 0.40, 0.80), 0.0),
    ("g2_right_wall", (0.2, 0.2, 0.2), (0.80, 0.25, 0.20), 0.0),
    ("g3_left_wall", (0.2, 0.2, 0.2), (0.25, 0.70, 0.30), 0.0),
    ("g4_glass_ball", (0.2, 0.2, 0.2), (0.85, 0.92, 0.95), 0.0),
    ("g5_glass_slab", (0.2, 0.2, 0.2), (0.75, 0.90, 0.85), 0.0),
    ("g6_box", (0.2, 0.2, 0.2), (0.90, 0.75, 0.15), 0.0),
    ("g7_box", (0.2, 0.2, 0.2), (0.70, 0.25, 0.75), 0.0),
    ("g8_mirror", (0.2, 0.2, 0.2), (0.70, 0.80, 0.90), 0.8),
]
# material index -> (d, Ni) of the MTL: d is OBJ's dissolve (1 = opaque), so the ball transmits 0.85 and the slab 0.8
GLASS_OF = {4: (0.15, 1.5), 5: (0.2, 1.33)}


def _wind_outwards(verts, faces):
    """The faces of a closed convex solid with every normal e1 x e2 pointing away from the solid's centroid."""
    verts, faces = np.asarray(verts, np.float64), np.array(faces, np.int64)
    c = verts[np.unique(faces)].mean(0)
    a, b, d = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    inward = np.einsum("ij,ij->i", np.cross(b - a, d - a), (a + b + d) / 3.0 - c) < 0
    faces[inward] = faces[inward][:, [0, 2, 1]]
    return verts, faces


def glass(outdir=None, scale=1.0):
    """Room [0,10]x[0,8]x[0,5] without a ceiling and without the wall x = 0 (behind the camera: see add_room): a matt
    floor, a blue back wall, a red and a green side wall.  In it a glass icosphere (d 0.15, Ni 1.5), a glass slab with
    all six faces (d 0.2, Ni 1.33) standing in front of two coloured boxes, and a mirror panel (r 0.8) before the back
    wall.  The glass solids are closed and wound outwards (refraction takes the side a ray enters from off the
    winding: DESIGN.md section 6.6).  ~10 000 triangles at scale 1."""
    mesh = Mesh()
    s = max(0.05, scale) ** 0.5
    n = max(2, int(20 * s))
    add_box(mesh, (0, 0, 0), (10, 8, 5), n, 0, faces="z")
    add_box(mesh, (0, 0, 0), (10, 8, 5), n, 1, faces="X")
    add_box(mesh, (0, 0, 0), (10, 8, 5), n, 2, faces="y")
    add_box(mesh, (0, 0, 0), (10, 8, 5), n, 3, faces="Y")
    level = max(1, min(7, int(round(4 + np.log(max(scale, 1e-3)) / np.log(4)))))  # (grows with the scale above 1 too)
    sv, sf = icosphere(level)
    mesh.add(*_wind_outwards(sv * 1.1 + np.array([5.5, 2.4, 1.35]), sf), 4)
    slab, nb = Mesh(), max(1, int(8 * s))
    add_box(slab, (4.6, 4.3, 0.02), (5.1, 7.1, 2.8), nb, 5)
    sv, sf, _ = slab.arrays()
    mesh.add(*_wind_outwards(sv, sf), 5)
    nb = max(1, int(6 * s))
    add_box(mesh, (6.6, 4.5, 0.0), (7.4, 5.3, 1.5), nb, 6, faces="xXyYZ")
    add_box(mesh, (6.9, 5.9, 0.0), (7.7, 6.7, 2.1), nb, 7, faces="xXyYZ")
    mesh.add(*grid_quad((9.9, 0.8, 0.5), (0, 3.0, 0), (0, 0, 3.0), max(1, int(8 * s)), max(1, int(8 * s))), 8)
    cams = {"ref": dict(eye=(0.6, 3.9, 2.0), look=(6.0, 4.3, 1.2), up=(0, 0, 1), near=0.1, far=100.0)}
    light_cam = dict(eye=(4.0, 4.0, 9.0), look=(4.0, 4.0, 0.0), up=(0, 1, 0), near=0.1, far=100.0)
    info = _finish(outdir, "glass%dk" % round(mesh.ntris() / 1000), mesh, MATERIALS_GLASS,
                   dict(cameras=cams, light_camera=light_cam, shading_light=(4.0, 4.0, 4.5), glass=GLASS_OF))
    d_ni = [GLASS_OF.get(k, (1.0, 1.0)) for k in range(len(MATERIALS_GLASS))]
    # what the loader makes of the MTL's 6-decimal text: transmit = (float)(1 - d), ior = (float)Ni
    info["transmit"] = np.array([1.0 - float("%.6f" % d) for d, _ in d_ni], dtype=np.float32)
    info["ior"] = np.array([float("%.6f" % ni) for _, ni in d_ni], dtype=np.float32)
    return info


MATERIALS_GLOSSY = [
    # name, Ka, Kd, reflect
    ("y0_floor_sharp", (0.2, 0.2, 0.2), (0.45, 0.45, 0.50), 0.6),
    ("y1_floor_satin", (0.2, 0.2, 0.2), (0.45, 0.45, 0.50), 0.6),
    ("y2_floor_rough", (0.2, 0.2, 0.2), (0.45, 0.45, 0.50), 0.6),
    ("y3_matte_wall", (0.2, 0.2, 0.2), (0.80, 0.78, 0.70), 0.0),
    ("y4_red", (0.2, 0.2, 0.2), (0.85, 0.15, 0.12), 0.0),
    ("y5_blue", (0.2, 0.2, 0.2), (0.12, 0.25, 0.85), 0.0),
    ("y6_yellow", (0.2, 0.2, 0.2), (0.90, 0.80, 0.15), 0.0),
    ("y7_column", (0.2, 0.2, 0.2), (0.70, 0.66, 0.60), 0.0),
]
# material index -> the MTL's sharpness (0..1000; 1000 is a mirror): the three strips of the floor
GLOSSY_SHARPNESS_OF = {0: 1000.0, 1: 700.0, 2: 300.0}
GLOSSY_STRIPS = ((0.0, 2.0), (2.0, 4.0), (4.0, 6.0))  # the strips' y ranges, in the order of the materials


def spread_from_sharpness(sh):
    """The spread of a material's reflection lobe from the MTL's sharpness:
    0.5 * (1 - clip(sh, 0, 1000) / 1000) ** 2, computed in float64 and returned as float32 -- sharpness 1000 gives 0, a
    mirror, sharpness 0 gives 0.5, the tangent of the lobe's half-angle.  The library only ever sees spreads as data."""
    sh = np.clip(np.asarray(sh, dtype=np.float64), 0.0, 1000.0)
    return (0.5 * (1.0 - sh / 1000.0) ** 2).astype(np.float32)


def glossy(outdir=None, scale=1.0):
    """Room [0,12]x[0,6]x[0,6] with a floor and one matte wall (x = 12) only: rays that climb or leave sideways leave the
    grid.  The floor is three strips along x, y in GLOSSY_STRIPS, of one Kd and r = 0.6 with sharpness 1000, 700 and 300.
    On every strip, in the same places, stands a row of six thin posts of alternating colours, and on the middle strip
    behind its row a column: the posts are narrower than the rough strip's lobe and wider than a pixel, so each strip
    shows them less crisp than the one before.  The camera looks along x down onto the floor in front of the posts.
    ~5 000 triangles at scale 1."""
    mesh = Mesh()
    s = max(0.05, scale) ** 0.5
    n = max(2, int(24 * s))
    for m, (y0, y1) in enumerate(GLOSSY_STRIPS):
        mesh.add(*grid_quad((0, y0, 0), (12, 0, 0), (0, y1 - y0, 0), n, max(1, n // 6)), m)
    mesh.add(*grid_quad((12, 0, 0), (0, 6, 0), (0, 0, 6), n, n), 3)
    nb = max(1, int(4 * s))
    for y0, _ in GLOSSY_STRIPS:
        for i in range(6):
            ya = y0 + 0.2 + 0.3 * i
            add_box(mesh, (8.0, ya, 0.0), (8.3, ya + 0.14, 2.6), nb, 4 + i % 3, faces="xXyYZ")
    add_cylinder(mesh, 10.0, 3.0, 0.0, 4.0, 0.35, max(6, int(24 * s)), max(2, int(8 * s)), 7)
    cams = {"ref": dict(eye=(0.3, 3.0, 2.5), look=(7.0, 3.0, 0.5), up=(0, 0, 1), near=0.1, far=100.0)}
    light_cam = dict(eye=(5.0, 3.0, 9.0), look=(5.0, 3.0, 0.0), up=(0, 1, 0), near=0.1, far=100.0)
    info = _finish(outdir, "glossy%dk" % round(mesh.ntris() / 1000), mesh, MATERIALS_GLOSSY,
                   dict(cameras=cams, light_camera=light_cam, shading_light=(5.0, 3.0, 5.0),
                        sharpness_of=GLOSSY_SHARPNESS_OF))
    # what the loader makes of the MTL: the written values, and its default 98 where there is no line
    info["sharpness"] = np.array([GLOSSY_SHARPNESS_OF.get(k, 98.0) for k in range(len(MATERIALS_GLOSSY))], dtype=np.float32)
    info["spread"] = spread_from_sharpness(info["sharpness"])
    return info


def weld(verts, tol=0.0):
    """One int32 key per vertex for Renderer(vertex_key=): the lowest index among the vertices
    equal to it, so that the generators' duplicated vertices -- every quad of add_box brings its own corners -- share their
    faces.  tol == 0 compares the float32 bit patterns, -0 equal to +0.  tol > 0 compares the coordinates rounded to
    multiples of tol: add_cylinder's seam columns (cos and sin of 0 and of 2 pi) differ in their last bits and need it."""
    v = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
    if not float(tol) >= 0.0:
        raise ValueError("tol must be a number not below 0, not %r" % (tol,))
    if len(v) == 0:
        return np.zeros(0, np.int32)
    if tol == 0:
        rows = v.view(np.uint32).copy()
        rows[rows == 0x80000000] = 0
    else:
        rows = np.rint(v.astype(np.float64) / float(tol))
        rows[rows == 0] = 0.0  # (-0 as +0)
        rows = rows.view(np.uint64)
    _, first, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    return first[np.asarray(inverse).reshape(-1)].astype(np.int32)


MATERIALS_SMOOTH = [
    # name, Ka, Kd, reflect
    ("s0_floor", (0.2, 0.2, 0.2), (0.62, 0.60, 0.55), 0.0),
    ("s1_back_wall", (0.2, 0.2, 0.2), (0.30, 0.40, 0.80), 0.0),
    ("s2_right_wall", (0.2, 0.2, 0.2), (0.80, 0.25, 0.20), 0.0),
    ("s3_left_wall", (0.2, 0.2, 0.2), (0.25, 0.70, 0.30), 0.0),
    ("s4_ball", (0.2, 0.2, 0.2), (0.85, 0.80, 0.70), 0.0),
    ("s5_column", (0.2, 0.2, 0.2), (0.70, 0.66, 0.60), 0.0),
    ("s6_box", (0.2, 0.2, 0.2), (0.90, 0.75, 0.15), 0.0),
]


def smooth(outdir=None, scale=1.0):
    """glass()'s room [0,10]x[0,8]x[0,5] with three solids for display(smooth=True): an
    icosphere(2) ball, whose 320 flat triangles are what smooth shading is for; a 32-segment column without caps, whose
    seam only a weld with a tolerance closes; and a box with 3 x 3 vertices per side, whose edges a crease angle must
    keep.  info["vertex_key"] is weld(verts, 1e-5); info["objects"] names the solids' face ranges [begin, end).  The
    solids are wound outwards.  The room's tessellation follows the scale, the solids do not."""
    mesh = Mesh()
    n = max(2, int(20 * max(0.05, scale) ** 0.5))
    add_box(mesh, (0, 0, 0), (10, 8, 5), n, 0, faces="z")
    add_box(mesh, (0, 0, 0), (10, 8, 5), n, 1, faces="X")
    add_box(mesh, (0, 0, 0), (10, 8, 5), n, 2, faces="y")
    add_box(mesh, (0, 0, 0), (10, 8, 5), n, 3, faces="Y")
    objects = {}
    begin = mesh.ntris()
    sv, sf = icosphere(2)
    mesh.add(*_wind_outwards(sv * 1.1 + np.array([5.5, 2.4, 1.35]), sf), 4)
    objects["sphere"] = (begin, mesh.ntris())
    begin = mesh.ntris()
    add_cylinder(mesh, 6.6, 5.6, 0.0, 3.2, 0.6, 32, 4, 5)
    objects["cylinder"] = (begin, mesh.ntris())
    begin = mesh.ntris()
    box = Mesh()
    add_box(box, (3.9, 3.7, 0.0), (4.9, 4.7, 1.0), 2, 6)
    bv, bf, _ = box.arrays()
    mesh.add(*_wind_outwards(bv, bf), 6)
    objects["box"] = (begin, mesh.ntris())
    cams = {"ref": dict(eye=(0.6, 3.9, 2.0), look=(6.0, 4.3, 1.2), up=(0, 0, 1), near=0.1, far=100.0)}
    light_cam = dict(eye=(4.0, 4.0, 9.0), look=(4.0, 4.0, 0.0), up=(0, 1, 0), near=0.1, far=100.0)
    info = _finish(outdir, "smooth%dk" % round(mesh.ntris() / 1000), mesh, MATERIALS_SMOOTH,
                   dict(cameras=cams, light_camera=light_cam, shading_light=(4.0, 4.0, 4.5)))
    info["vertex_key"] = weld(info["verts"], 1e-5)
    info["objects"] = objects
    return info


DEPTH_POSTS = ((5.0, -0.8), (8.0, 0.45), (12.0, 0.0), (18.0, -0.4), (26.0, 0.8))  # distance along the view, side


def depth(outdir=None, scale=1.0):
    """A floor [2,30]x[0,26] at z = 0 (in front of the eye only: the primary pass takes |t|) and five identical thin
    posts, 0.5 x 0.5 x 5, at the distances of DEPTH_POSTS along the view axis +x of a camera at (1, 13, 2.5), each moved
    sideways by its second entry times a third of its distance so that none hides another.  The default look-at is the
    middle post's axis: a lens focused there (Renderer.display(..., dof=S)) keeps it sharp and blurs the near and the far
    ones.  info["posts"]: per post (first face, one past its last face, distance).  ~700 triangles at scale 1."""
    mesh = Mesh()
    s = max(0.05, scale) ** 0.5
    n = max(2, int(12 * s))
    mesh.add(*grid_quad((2, 0, 0), (28, 0, 0), (0, 26, 0), n, n), 0)
    nb = max(1, int(3 * s))
    posts = []
    for dist, side in DEPTH_POSTS:
        first = mesh.ntris()
        x, y = 1.0 + dist, 13.0 + side * dist / 3.0
        add_box(mesh, (x - 0.25, y - 0.25, 0.0), (x + 0.25, y + 0.25, 5.0), nb, 5, faces="xXyYZ")
        posts.append((first, mesh.ntris(), dist))
    cams = {"ref": dict(eye=(1.0, 13.0, 2.5), look=(13.0, 13.0, 2.5), up=(0, 0, 1), near=0.1, far=100.0)}
    # the lights stand behind and above the eye: the faces the camera sees are lit alike, post after post
    light_cam = dict(eye=(-8.0, 13.0, 16.0), look=(14.0, 13.0, 0.0), up=(0, 1, 0), near=0.1, far=100.0)
    info = _finish(outdir, "depth", mesh, MATERIALS_ROOM,
                   dict(cameras=cams, light_camera=light_cam, shading_light=(-10.0, 13.0, 8.0)))
    info["posts"] = posts
    return info


def planar_uvs(verts, faces, scale=1.0):
    """Texture coordinates for any mesh: every face is projected along the axis its normal is closest to -- (y, z) for x,
    (x, z) for y, (x, y) for z -- and the two coordinates are multiplied by scale (texture repeats per unit of length).
    Returns (uvs float32 [3F, 2], uv_faces int32 [F, 3]): one uv per corner, uv_faces[f] = (3f, 3f + 1, 3f + 2)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    c = v[f]
    axis = np.argmax(np.abs(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])), axis=1)
    keep = np.array([[1, 2], [0, 2], [0, 1]])[axis]
    uv = np.take_along_axis(c, np.repeat(keep[:, None, :], 3, 1), axis=2) * float(scale)
    return uv.reshape(-1, 2).astype(np.float32), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)


def checker_texture(size, cells, a=(235, 235, 235), b=(40, 40, 40)):
    """A size x size checkerboard of cells x cells squares, uint8 [size, size, 3]."""
    i = np.arange(size) * cells // size
    on = ((i[:, None] + i[None, :]) & 1).astype(bool)
    return np.where(on[..., None], np.uint8(b), np.uint8(a)).astype(np.uint8)


def stripes_texture(size, n, a=(230, 200, 60), b=(30, 60, 160)):
    """A size x size texture of n vertical stripes (constant along v), uint8 [size, size, 3]."""
    on = ((np.arange(size) * n // size) & 1).astype(bool)
    return np.repeat(np.where(on[:, None], np.uint8(b), np.uint8(a))[None], size, 0).astype(np.uint8)


MATERIALS_TEXTURED = [
    ("t0_floor", (0.2, 0.2, 0.2), (0.90, 0.90, 0.90), 0.0),
    ("t1_wall", (0.2, 0.2, 0.2), (0.95, 0.90, 0.85), 0.0),
    ("t2_box_plain", (0.2, 0.2, 0.2), (0.80, 0.25, 0.20), 0.0),
    ("t3_box_striped", (0.2, 0.2, 0.2), (1.00, 1.00, 1.00), 0.0),
]


def textured(outdir=None, scale=1.0):
    """A scene for display(textures=True).  A floor [1, 200] x [-60, 60] at z = 0 that runs to
    the horizon under a checker of 2 x 2 texels that repeats 16 times per unit of length -- the aliasing case; a wall at
    x = 12 seen head-on under an 8 x 8 checker that covers it once -- the magnification case; and two boxes side by side, one
    of an untextured material, one striped.  info: uvs, uv_faces, textures (a list of uint8 arrays), mat_texture (one int per
    material, -1: none) and texture_files {material: (file name, array)} for write_scene."""
    mesh = Mesh()
    n = max(2, int(8 * max(0.05, scale) ** 0.5))
    mesh.add(*grid_quad((1, -60, 0), (199, 0, 0), (0, 120, 0), n, n), 0)
    mesh.add(*grid_quad((12, 2.0, 0), (0, 5, 0), (0, 0, 4), 2, 2), 1)
    add_box(mesh, (6.0, -3.2, 0.0), (7.2, -2.0, 1.2), 1, 2, faces="xyYZ")
    add_box(mesh, (6.0, -1.6, 0.0), (7.2, -0.4, 1.2), 1, 3, faces="xyYZ")
    verts, faces, matidx = mesh.arrays()
    uvs, uv_faces = planar_uvs(verts, faces, 1.0)
    per_material = {0: 16.0, 1: 0.2, 2: 1.0, 3: 2.5}
    for m, k in per_material.items():
        uvs[uv_faces[matidx == m].reshape(-1)] *= np.float32(k)
    uv_faces[matidx == 2] = -1
    textures = [checker_texture(2, 2), checker_texture(8, 8, (250, 240, 200), (120, 30, 30)), stripes_texture(64, 8)]
    files = {0: ("floor_checker.ppm", textures[0]), 1: ("wall_checker.ppm", textures[1]), 3: ("box_stripes.ppm", textures[2])}
    cams = {"ref": dict(eye=(0.0, 0.0, 1.5), look=(12.0, 1.0, 1.2), up=(0, 0, 1), near=0.1, far=400.0)}
    light_cam = dict(eye=(5.0, 0.0, 12.0), look=(8.0, 0.0, 0.0), up=(0, 1, 0), near=0.1, far=400.0)
    info = _finish(outdir, "textured", mesh, MATERIALS_TEXTURED,
                   dict(cameras=cams, light_camera=light_cam, shading_light=(4.0, -2.0, 6.0), uvs=uvs, uv_faces=uv_faces,
                        texture_files=files))
    info["textures"] = textures
    info["mat_texture"] = np.int32([0, 1, -1, 2])
    return info


def ao_directions(S):
    """The S local directions of the ambient-occlusion hemisphere: a deterministic
    cosine-weighted spiral, r = sqrt((s + 1/2) / S), phi = s * pi * (3 - sqrt(5)), direction
    (r cos phi, r sin phi, sqrt(1 - r^2)) with z along the normal.  Computed in float64 and returned as float32 [S, 3]:
    the library only ever sees these floats as data."""
    s = np.arange(int(S), dtype=np.float64)
    r = np.sqrt((s + 0.5) / float(S))
    phi = s * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - r * r)], 1).astype(np.float32)


AREA_SET_RANK = {1: (0,), 4: (0, 2, 3, 1), 16: (0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5)}  # 4 x 4: Bayer


def _spiral_directions(S, turn):
    """ao_directions' directions with `turn` added to every angle."""
    s = np.arange(int(S), dtype=np.float64)
    r = np.sqrt((s + 0.5) / float(S))
    phi = s * (np.pi * (3.0 - np.sqrt(5.0))) + turn
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - r * r)], 1).astype(np.float32)


def ao_direction_sets(S, sets):
    """The interleaved direction sets of the ambient-occlusion hemisphere: sets = 1, 4 or 16 for a
    tile of 1 x 1, 2 x 2 or 4 x 4 pixels; set k (row-major in the tile) is ao_directions' formula with
    phi = s * pi * (3 - sqrt(5)) + 2 pi * rank[k] / sets, rank = AREA_SET_RANK[sets], as area_sample_sets turns the disk.
    Computed in float64 and returned as float32 [sets, S, 3]; set 0 is ao_directions bit for bit."""
    if sets not in AREA_SET_RANK:
        raise ValueError("sets must be 1, 4 or 16, not %r" % (sets,))
    return np.stack([_spiral_directions(S, 2.0 * np.pi * rank / float(sets)) for rank in AREA_SET_RANK[sets]])


def glossy_points(S):
    """The S points of a reflection lobe in the unit disk: the (x, y) of ao_directions, float32
    [S, 2].  Times a material's spread they tilt the mirror direction."""
    return np.ascontiguousarray(ao_directions(S)[:, :2])


def glossy_point_sets(S, sets):
    """The interleaved point sets of the reflection lobes: the (x, y) of ao_direction_sets(S, sets) -- the same spiral, the
    same AREA_SET_RANK turns --, float32 [sets, S, 2]; set 0 is glossy_points bit for bit."""
    return np.ascontiguousarray(ao_direction_sets(S, sets)[:, :, :2])


def _disk_points(S, centre, axis, radius, turn):
    """area_samples' points with `turn` added to every angle."""
    c = np.asarray(centre, np.float64).reshape(3)
    a = np.asarray(axis, np.float64).reshape(3)
    a = a / np.sqrt((a * a).sum())
    k = int(np.argmin(np.abs(a)))  # (the first of equal minima)
    e = np.zeros(3)
    e[k] = 1.0
    T = np.cross(a, e)
    T = T / np.sqrt((T * T).sum())
    B = np.cross(a, T)
    s = np.arange(int(S), dtype=np.float64)
    r = float(radius) * np.sqrt((s + 0.5) / float(S))
    phi = s * (np.pi * (3.0 - np.sqrt(5.0))) + turn
    return (c + (r * np.cos(phi))[:, None] * T + (r * np.sin(phi))[:, None] * B).astype(np.float32)


def area_sample_sets(S, sets, centre, axis, radius):
    """The interleaved sample sets of an area light's disk: sets = 1, 4 or 16 for a tile of
    1 x 1, 2 x 2 or 4 x 4 pixels; set k (row-major in the tile) is area_samples' formula with
    phi = s * pi * (3 - sqrt(5)) + 2 pi * rank[k] / sets, rank = AREA_SET_RANK[sets]: neighbouring pixels' spirals are
    turned against each other by as much as the tile allows.  Computed in float64 and returned as float32 [sets, S, 3];
    set 0 is area_samples bit for bit."""
    if sets not in AREA_SET_RANK:
        raise ValueError("sets must be 1, 4 or 16, not %r" % (sets,))
    return np.stack([_disk_points(S, centre, axis, radius, 2.0 * np.pi * rank / float(sets)) for rank in AREA_SET_RANK[sets]])


def area_samples(S, centre, axis, radius):
    """The S points of an area light's disk: radius `radius` around `centre`, perpendicular to
    `axis`.  With a = axis / |axis|, k the index of the smallest |a[k]| (ties go to the lowest k), T = normalize(a x e_k)
    and B = a x T: r = radius * sqrt((s + 1/2) / S), phi = s * pi * (3 - sqrt(5)), point
    centre + r cos phi * T + r sin phi * B.  Computed in float64 and returned as float32 [S, 3]: the library only ever
    sees these floats as data."""
    return _disk_points(S, centre, axis, radius, 0.0)  # (phi + 0.0 is phi: the floats are what they were)


def _aa_points(S, shift_x, shift_y):
    """aa_offsets' points moved by (shift_x, shift_y) of a pixel and wrapped back into it."""
    S = int(S)
    s = np.arange(S, dtype=np.int64)
    inverse = np.zeros(S, np.float64)  # the radical inverse of s in base 2 (van der Corput)
    digit, rest = 0.5, s.copy()
    while rest.any():
        inverse += digit * (rest & 1)
        rest >>= 1
        digit *= 0.5
    u = np.stack([(s + 0.5) / float(S) + shift_x, inverse + 0.5 / float(S) + shift_y], 1)
    out = ((u % 1.0) - 0.5).astype(np.float32)
    return np.clip(out, np.float32(-0.5), np.nextafter(np.float32(0.5), np.float32(0.0)))


def aa_offsets(S):
    """The S sub-pixel offsets of the anti-aliasing's eye rays, in [-0.5, 0.5) around the point
    the pixel's own ray goes through: sample s lies at ((s + 1/2) / S, vdc(s) + 1 / (2 S)) - 1/2, vdc the radical inverse in
    base 2 (the Hammersley set): every one of the S column strata holds one point, and for S a power of two every one of
    the S row strata does.  S = 1 gives (0, 0), the pixel's own ray.  Computed in float64 and returned as float32 [S, 2]:
    the library only ever sees these floats as data."""
    return _aa_points(S, 0.0, 0.0)


def aa_offset_sets(S, sets):
    """The interleaved offset sets of the anti-aliasing: sets = 1, 4 or 16 for a tile of 1 x 1,
    2 x 2 or 4 x 4 pixels; set k (row-major in the tile) is aa_offsets' set moved by rank[k] / (sets + 1) of a column
    stratum and by rank[sets - 1 - k] / (sets + 1) of one S-th of the pixel's height and wrapped back into the pixel, rank =
    AREA_SET_RANK[sets] as area_sample_sets turns the disk: the sets of a tile together hold sets * S different columns,
    every set keeps one point per column stratum, and no point lies on a stratum's edge (sets + 1 is odd).
    float32 [sets, S, 2]; set 0 is aa_offsets bit for bit."""
    if sets not in AREA_SET_RANK:
        raise ValueError("sets must be 1, 4 or 16, not %r" % (sets,))
    rank = AREA_SET_RANK[sets]
    step = 1.0 / (float(sets + 1) * float(int(S)))
    return np.stack([_aa_points(S, rank[k] * step, (rank[sets - 1 - k] * step) if k else 0.0) for k in range(sets)])


def lens_sample_sets(S, sets):
    """The interleaved sample sets of the depth of field's lens rays: per sample
    (sx, sy, lu, lv) -- aa_offset_sets(S, sets)' sub-pixel offset and glossy_point_sets(S, sets)' point of the unit disk,
    the spiral turned per set by the AREA_SET_RANK turns.  float32 [sets, S, 4]."""
    return np.ascontiguousarray(np.concatenate([aa_offset_sets(S, sets), glossy_point_sets(S, sets)], 2), dtype=np.float32)


def temporal_sets(table16, sets, frame):
    """Frame `frame`'s table of a temporal sequence, from a table of 16 sets
    (ao_direction_sets(S, 16), area_sample_sets(S, 16, ...), the indirect light's directions): entry k of the tile of
    sets = 1, 4 or 16 pixels is set (k * (16 // sets) + frame) % 16.  Over 16 frames every entry goes through all 16 sets,
    and in any one frame the entries of a tile hold different sets.  [sets, S, c] in table16's type; a copy."""
    if sets not in AREA_SET_RANK:
        raise ValueError("sets must be 1, 4 or 16, not %r" % (sets,))
    table16 = np.asarray(table16)
    if table16.shape[0] != 16:
        raise ValueError("a table of 16 sets is expected, not %d" % table16.shape[0])
    pick = [(k * (16 // sets) + int(frame)) % 16 for k in range(sets)]
    return np.ascontiguousarray(table16[pick])
