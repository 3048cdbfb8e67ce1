"""Texture mapping: the loader's texture coordinates and names, ugrt_read_ppm, ugrt_texture_set,
ugrt_texture_albedo, ugrt_texture_shade and ugrt_texture_shade_lights, against tests/texture_ref.c (one loop per texel, one
per pixel) and numpy, to the bit.

  CPU  the prototypes; the OBJ / MTL grammar on hand-written files (pinned to obj_parser.cpp:16-25, 52-90 by reading it);
       the PPM reader; both parsers under ASan + UBSan as a stand-alone program; the checker against its definition.
  GPU  every level of five textures in one atlas; the albedo on a synthetic 64 x 40 g-buffer; the two shading calls against
       the oracle's with one material per pixel, and against ugrt_shade_simple / ugrt_shade_lights; the errors.

A band of a context is whole tile rows (8 pixel rows), so the band of the g-buffer tests starts and ends between rows."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_reflect_depth as RD
import test_reflect_shadows as RS
from test_lights import LT  # noqa: F401  (fixture: the checker of the several-lights shading)
from test_smooth import assert_same

HERE = os.path.dirname(os.path.abspath(__file__))
_p, _f32, _i32, bits = RD._p, RD._f32, RD._i32, RD.bits
CALLS = ("ugrt_texture_set", "ugrt_texture_get_level", "ugrt_texture_albedo", "ugrt_texture_shade", "ugrt_texture_shade_spotlight",
         "ugrt_texture_shade_lights")
HOST_CALLS = ("ugrt_scene_uvlist", "ugrt_scene_uv_facelist", "ugrt_scene_texture_name", "ugrt_scene_texture_dir", "ugrt_read_ppm")
SIZES = ((1, 1), (1, 7), (5, 3), (64, 64), (257, 129))  # (w, h) of the five textures
GW, GH = 64, 40


class TextureRef:
    def __init__(self, lib):
        self.lib = lib

    def chain(self, tex):
        """[(w, h, words)] per level of the uint8 texture [H, W, 3]."""
        tex = np.ascontiguousarray(tex, np.uint8)
        h, w = tex.shape[:2]
        out = np.zeros(self.lib.tex_chain_words(w, h), np.uint32)
        dims = np.zeros(64, np.int32)
        self.lib.tex_chain(_p(tex), C.c_int(w), C.c_int(h), _p(out), _p(dims))
        levels, at = [], 0
        for l in range(self.lib.tex_levels(w, h)):
            lw, lh = int(dims[2 * l]), int(dims[2 * l + 1])
            levels.append((lw, lh, out[at:at + lw * lh].copy()))
            at += lw * lh
        assert at == len(out)
        return levels

    def directions(self, eye, nodes, W, H, strict, fcol, frow):
        fcol, frow = _f32(fcol), _f32(frow)
        d = np.zeros(3 * len(fcol), np.float32)
        self.lib.tex_directions(_p(_f32(eye)), _p(_f32(nodes)), C.c_int(W), C.c_int(H), C.c_int(strict), C.c_int(len(fcol)),
                                _p(fcol), _p(frow), _p(d))
        return d.reshape(-1, 3)

    def albedo(self, g, textures, max_aniso, lod_bias, strict=0, p0=0, n=None, fill=7.0):
        """(albedo words over the whole frame -- `fill` outside the band --, dbg [N, 4])."""
        N = g["N"]
        n = N if n is None else n
        out = np.full(3 * N, fill, np.float32)
        dbg = np.zeros(4 * N, np.int32)
        wh = _i32([d for t in textures for d in (t.shape[1], t.shape[0])] or [0])
        rgb = np.concatenate([np.ascontiguousarray(t, np.uint8).reshape(-1) for t in textures] or [np.zeros(1, np.uint8)])
        self.lib.tex_albedo(_p(_f32(g["t"])), _p(_f32(g["dirs"])), _p(_i32(g["ids"])), _p(_f32(g["cam"])), _p(_f32(g["verts"])),
                            _p(_i32(g["faces"])), _p(_f32(g["uvs"])), C.c_int(len(g["uvs"]) // 2), _p(_i32(g["uv_faces"])),
                            _p(_i32(g["mat_idx"])), _p(_f32(g["mat_list"])), C.c_int(len(g["mat_list"]) // 6),
                            _p(_i32(g["mat_texture"])), C.c_int(len(textures)), _p(wh), _p(rgb), _p(_f32(g["cc"][:3])),
                            _p(_f32(g["nodes"])), C.c_int(g["W"]), C.c_int(g["H"]), C.c_int(strict), C.c_int(max_aniso),
                            C.c_int(lod_bias), _p(out), C.c_int(p0), C.c_int(n), _p(dbg))
        return out, dbg.reshape(-1, 4)

    def albedo_super(self, g, textures, sub):
        """The albedo of sub x sub eye rays per pixel, bilinear on level 0, averaged (the reference of the aliasing figure)."""
        N = g["N"]
        out = np.zeros(3 * N, np.float32)
        wh = _i32([d for t in textures for d in (t.shape[1], t.shape[0])])
        rgb = np.concatenate([np.ascontiguousarray(t, np.uint8).reshape(-1) for t in textures])
        self.lib.tex_albedo_super(_p(_f32(g["t"])), _p(_f32(g["dirs"])), _p(_i32(g["ids"])), _p(_f32(g["cam"])), _p(_f32(g["verts"])),
                                  _p(_i32(g["faces"])), _p(_f32(g["uvs"])), C.c_int(len(g["uvs"]) // 2), _p(_i32(g["uv_faces"])),
                                  _p(_i32(g["mat_idx"])), _p(_f32(g["mat_list"])), C.c_int(len(g["mat_list"]) // 6),
                                  _p(_i32(g["mat_texture"])), C.c_int(len(textures)), _p(wh), _p(rgb), _p(_f32(g["cc"][:3])),
                                  _p(_f32(g["nodes"])), C.c_int(g["W"]), C.c_int(g["H"]), C.c_int(sub), _p(out), C.c_int(0), C.c_int(N))
        return out


@pytest.fixture(scope="session")
def TX(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("texture_ref") / "libtexture_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "texture_ref.c"), "-lm"], check=True, capture_output=True)
    lib = C.CDLL(out)
    lib.tex_chain_words.restype = lib.tex_levels.restype = C.c_int
    lib.tex_chain_words.argtypes = lib.tex_levels.argtypes = [C.c_int, C.c_int]
    return TextureRef(lib)


def textures(seed=618):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for w, h in SIZES]


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    header = open(os.path.join(RD.ROOT, "include", "ugrt.h")).read()
    for name in CALLS + HOST_CALLS:
        assert hasattr(lib, name) and name in ugrt.PROTOTYPES and name + "(" in header, name
    for name in CALLS:
        assert callable(getattr(ugrt.Context, name[5:]))
    for name in ("h_uvlist", "h_uvfacelist", "h_texturelist"):
        assert isinstance(getattr(ugrt.Model, name), property)
    assert lib.ugrt_version() == 105


OBJ = """mtllib m.mtl
v 0 0 0
v 1 0 0
v 0 1 0
v 1 1 0
vt 0.25
vt 0.5 0.75
usemtl kd
f 1 2 3
f 1/1 2/2 3/1
vt 1.5 -2.25 9.0
f 1//1 2//1 3//1
f 1/3/1 2/2/1 3/1/1
usemtl ka
f 1/1 2 3//2
f 1/-1 2/-3 3/-4
f 1/0 2/4 3/3
vt 7 8
f 1/4 2/5 3/-1
usemtl both
f 1/1 2/2 3/3 4/4
usemtl opt
f 4/4 3/3 2/2
"""
MTL = """newmtl kd
Kd 0.1 0.2 0.3
map_Kd wood.ppm
newmtl ka
map_Ka  \tstone.ppm
newmtl both
map_Ka a.ppm
map_Kd d.ppm
map_Ka again.ppm
newmtl opt
map_Kd -s 2 2 scaled.ppm
newmtl none
Kd 1 1 1
"""
UVS = [0.25, 0.0, 0.5, 0.75, 1.5, -2.25, 7.0, 8.0]
UV_FACES = [[-1, -1, -1], [0, 1, 0], [-1, -1, -1], [2, 1, 0], [0, -1, -1], [2, 0, -1], [-1, 3, 2], [3, -1, 3], [0, 1, 2], [3, 2, 1]]
NAMES = ["wood.ppm", "stone.ppm", "d.ppm", "", ""]


def _strip_t(text):
    """The OBJ with the /t parts of its face tokens taken out: v/t -> v, v/t/n -> v//n."""
    out = []
    for line in text.splitlines(True):
        if line.startswith("f "):
            toks = []
            for tok in line.split():
                parts = tok.split("/")
                toks.append(tok if len(parts) == 1 else parts[0] if len(parts) == 2 else parts[0] + "//" + parts[2])
            line = " ".join(toks) + line[len(line.rstrip("\r\n")):]
        out.append(line)
    return "".join(out)


def _load(ugrt, d, obj, mtl, name="a.obj"):
    d.mkdir(exist_ok=True)
    (d / name).write_bytes(obj.encode())
    (d / "m.mtl").write_bytes(mtl.encode())
    m = ugrt.Model()
    m.load_model(d / name)
    return m


@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_the_loader_keeps_texture_coordinates_indices_and_names(ugrt, tmp_path, eol):
    obj, mtl = OBJ.replace("\n", eol), MTL.replace("\n", eol)
    m = _load(ugrt, tmp_path / "full", obj, mtl)
    np.testing.assert_array_equal(m.h_uvlist, np.float32(UVS))
    np.testing.assert_array_equal(m.h_uvfacelist.reshape(-1, 3), np.int32(UV_FACES))
    assert m.h_texturelist == NAMES
    assert m.texture_dir == str(tmp_path / "full") + "/"
    assert ugrt.lib.ugrt_scene_texture_name(m._h, -1) == b"" and ugrt.lib.ugrt_scene_texture_name(m._h, 5) == b""
    # the lists the loader had before are those of the same file without its /t parts
    assert "/" in obj and _strip_t("f 1/2 3/4/5 6//7 8\n") == "f 1 3//5 6//7 8\n"
    s = _load(ugrt, tmp_path / "stripped", _strip_t(obj), mtl)
    for name in ("h_vertexlist", "h_facelist", "h_materiallist_index", "h_reflectlist", "h_transmitlist", "h_iorlist", "h_sharpnesslist"):
        np.testing.assert_array_equal(getattr(m, name), getattr(s, name), err_msg=name)
    assert (s.h_uvfacelist == -1).all() and len(s.h_uvlist) == 8 and m.num_faces == 10
    np.testing.assert_array_equal(m.h_materiallist_index, [0, 0, 0, 0, 1, 1, 1, 1, 2, 3])
    np.testing.assert_array_equal(m.h_facelist.reshape(-1, 3)[8:], [[0, 1, 2], [3, 2, 1]])  # the quad's fourth token is dropped
    # no mtllib, no vt: nothing, and no failure
    e = ugrt.Model()
    (tmp_path / "bare.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/1 2/2 3/3\n")
    e.load_model(tmp_path / "bare.obj")
    assert len(e.h_uvlist) == 0 and list(e.h_uvfacelist) == [-1, -1, -1] and e.h_texturelist == [] and e.texture_dir == ""
    # a cached scene has no uvs and no textures
    (tmp_path / "uv.obj").write_text("mtllib full/m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nf 1/1 2/2 3/3\n")
    e.load_model(tmp_path / "uv.obj")
    assert list(e.h_uvfacelist) == [0, 1, 2] and e.h_texturelist == NAMES and e.texture_dir == str(tmp_path) + "/full/"
    e.save_cache(tmp_path / "scene.bin")
    c = ugrt.Model()
    c.load_cache(tmp_path / "scene.bin")
    assert c.num_faces == 1 and len(c.h_uvlist) == 0 and list(c.h_uvfacelist) == [-1, -1, -1] and c.h_texturelist == [""] * 5


def _ppm(path, magic, w, h, maxval, samples, comment=True, sep="\n"):
    samples = np.asarray(samples, np.uint8).reshape(-1)
    head = "%s\n%s%d %s%d\n%s%d" % (magic, "# made by hand\n" if comment else "", w, "#w\n" if comment else "", h,
                                    "# the maxval\n" if comment else "", maxval)
    body = samples.tobytes() if magic == "P6" else (" ".join(str(int(v)) for v in samples) + "\n").encode()
    with open(path, "wb") as fh:
        fh.write(head.encode() + sep.encode() + body)
    return str(path)


def test_read_ppm(ugrt, tmp_path):
    rng = np.random.RandomState(619)
    img = rng.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    ugrt.write_ppm(tmp_path / "w.ppm", img)
    np.testing.assert_array_equal(ugrt.read_ppm(tmp_path / "w.ppm"), img)
    for magic in ("P3", "P6"):
        for maxval in (1, 15, 255):
            raw = rng.randint(0, maxval + 1, (3, 4, 3)).astype(np.uint8)
            got = ugrt.read_ppm(_ppm(tmp_path / "a.ppm", magic, 4, 3, maxval, raw))
            np.testing.assert_array_equal(got, (raw.astype(np.int64) * 255 // maxval).astype(np.uint8), err_msg="%s %d" % (magic, maxval))
        assert ugrt.read_ppm(_ppm(tmp_path / "b.ppm", magic, 1, 1, 255, [1, 2, 3], comment=False)).tolist() == [[[1, 2, 3]]]
        tall = rng.randint(0, 256, (4096, 1, 3)).astype(np.uint8)
        np.testing.assert_array_equal(ugrt.read_ppm(_ppm(tmp_path / "c.ppm", magic, 1, 4096, 255, tall)), tall)
    w, h = C.c_int(), C.c_int()
    buf = np.full(64, 0xA5, np.uint8)

    def rc(path, rgb=None, cap=0, wp=C.byref(w), hp=C.byref(h)):
        return ugrt.lib.ugrt_read_ppm(None if path is None else str(path).encode(), wp, hp, None if rgb is None else _p(rgb), cap)

    good = _ppm(tmp_path / "g.ppm", "P6", 2, 2, 255, np.arange(12))
    assert rc(good) == 0 and (w.value, h.value) == (2, 2)
    assert rc(good, buf, 12) == 0 and list(buf[:12]) == list(range(12)) and (buf[12:] == 0xA5).all()
    assert rc(None) == ugrt.UGRT_EINVAL and rc(good, wp=None) == ugrt.UGRT_EINVAL and rc(good, hp=None) == ugrt.UGRT_EINVAL
    bad = {
        "missing": str(tmp_path / "nowhere.ppm"),
        "wide": _ppm(tmp_path / "e1.ppm", "P6", 4097, 1, 255, np.zeros(3 * 4097)),
        "high": _ppm(tmp_path / "e2.ppm", "P3", 1, 4097, 255, [0]),
        "zero": _ppm(tmp_path / "e3.ppm", "P6", 0, 1, 255, []),
        "maxval 256": _ppm(tmp_path / "e4.ppm", "P3", 1, 1, 256, [1, 2, 3]),
        "maxval 65535": _ppm(tmp_path / "e5.ppm", "P6", 1, 1, 65535, [1, 2, 3, 4, 5, 6]),
        "maxval 0": _ppm(tmp_path / "e6.ppm", "P6", 1, 1, 0, [1, 2, 3]),
        "short P6": _ppm(tmp_path / "e7.ppm", "P6", 2, 2, 255, np.arange(11)),
        "short P3": _ppm(tmp_path / "e8.ppm", "P3", 2, 2, 255, np.arange(11)),
        "sample above maxval P3": _ppm(tmp_path / "e9.ppm", "P3", 1, 1, 15, [1, 16, 3]),
        "sample above maxval P6": _ppm(tmp_path / "e10.ppm", "P6", 1, 1, 15, [1, 16, 3]),
        "P5": _ppm(tmp_path / "e11.ppm", "P5", 1, 1, 255, [1, 2, 3]),
        "a letter": _ppm(tmp_path / "e12.ppm", "P3", 1, 1, 255, [1, 2, 3]),
        "huge number": str(tmp_path / "e13.ppm"),
        "empty": str(tmp_path / "e14.ppm"),
        "no space behind the maxval": _ppm(tmp_path / "e15.ppm", "P6", 1, 1, 255, [1, 2, 3], sep=""),
    }
    open(bad["a letter"], "wb").write(b"P3\n1 1\n255\n1 x 3\n")
    open(bad["huge number"], "wb").write(b"P6\n99999999999999999999 1\n255\n")
    open(bad["empty"], "wb").write(b"")
    for what, path in bad.items():
        buf[:] = 0xA5
        assert rc(path, buf, 64) == ugrt.UGRT_EIO, what
        assert ugrt.lib.ugrt_last_error().startswith(b"read_ppm"), what
        if "above" not in what and "short" not in what and what != "a letter":
            assert (buf == 0xA5).all(), what
    buf[:] = 0xA5
    assert rc(good, buf, 11) == ugrt.UGRT_EIO and (buf == 0xA5).all()  # a capacity below 3 w h
    assert rc(bad["short P6"]) == 0  # the size alone reads the header only


def test_the_parsers_run_clean_under_asan_and_ubsan(ugrt, tmp_path):
    """A stand-alone program (tests/texture_parsers_main.cpp + ugrt_host.cpp, -fsanitize=address,undefined) over malformed
    and well-formed PPMs and OBJs: exit status 0 and no report.  The sanitizers' runtimes are linked statically, so the
    program starts whatever the environment preloads, and the environment is passed on as it is."""
    gxx = shutil.which("g++")
    # (a missing sanitizer fails the test: it is the parsers' only run under one, and a skip would hide that it did not happen)
    assert gxx is not None, "g++ is needed for the sanitizer build of the two parsers"
    asan = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    assert os.path.isabs(asan) and os.path.exists(asan), "g++ has no libasan here: the parsers cannot be run under ASan"
    exe = str(tmp_path / "parsers")
    csrc = os.path.join(RD.ROOT, "uniformgrid-raytracing_amd", "csrc")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all",
                    "-ffp-contract=off",
                    "-I", os.path.join(RD.ROOT, "include"), "-I", csrc, "-o", exe, os.path.join(HERE, "texture_parsers_main.cpp"),
                    os.path.join(csrc, "ugrt_host.cpp")], check=True, capture_output=True)
    files = []
    d = tmp_path / "files"
    d.mkdir()
    for k, data in enumerate((b"", b"P", b"P6", b"P6\n", b"P6\n#", b"P6\n# never ends", b"P6 1", b"P6\n1 1", b"P6\n1 1\n255", b"P6\n1 1\n255\n",
                              b"P6\n1 1\n255\n\x01\x02", b"P6\n1 1\n255\n\x01\x02\x03", b"P6\n2 2\n15\n" + bytes(range(12)) + b"\xff" * 40,
                              b"P3\n2 1\n255\n1 2 3 4 5", b"P3\n2 1\n255\n1 2 3 4 5 6", b"P3\n2 1\n255\n1 2 3 4 5 6 7 8", b"P3\n1 1\n7\n1 2 9\n",
                              b"P3\n1 1\n255\n-1 2 3\n", b"P3 4096 4096 255 1", b"P6 4097 4097 255\n", b"P6\n4294967297 1\n255\n\x00\x00\x00",
                              b"P6\n1 1\n255#c\n\x01\x02\x03", b"P3\n1 1\n255#c\n1 2#x\n3", b"P6\n 3 \t2\r\n255\r" + bytes(range(18)),
                              b"P7\n1 1\n255\n\x01\x02\x03", b"\x00" * 600, b"P6\n1 1\n" + b"9" * 600)):
        files.append(d / ("f%02d.ppm" % k))
        files[-1].write_bytes(data)
    long_token = "f " + "/".join(["1"] * 300) + " 2/ 3/-\n"
    objs = (OBJ, OBJ.replace("\n", "\r\n"), "f\nf 1\nf / // /// 1/ /1 1//\nvt\nvt x\nvt 1e999 -1e999\nf 1/1 1/1 1/1\n",
            "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\n" + "f 1/99999999999 2/-99999999999 3/2147483648\n" + long_token,
            "mtllib m.mtl\nmtllib\nusemtl\nv 1 2 3\nf 1/1/1/1/1 1/a 1/-0\n", "vt 1 2\n" * 3 + "v 0 0 0\n" + "f 1/3 1/2 1/1 1/0 1/-1 1/-2 1/-3 1/-4\n")
    for k, text in enumerate(objs):
        files.append(d / ("m%02d.obj" % k))
        files[-1].write_bytes(text.encode())
    (d / "m.mtl").write_bytes((MTL + "map_Kd\nmap_Ka\nnewmtl\nmap_Kd " + "x" * 700 + "\nnewmtl z\nmap_Kd \r\n").encode())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe] + [str(f) for f in files], capture_output=True, text=True, env=env, cwd=str(d), timeout=120)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "Sanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert out.count("read_ppm") + out.count("load_model") == len(files) and "done" in out
    assert "f11.ppm: read_ppm 0 (1 x 1), full 0, a byte short 4" in out and "m00.obj: load_model 0, 4 vertices, 10 faces, 4 vt, " in out


def test_the_checkers_mip_chain_is_what_the_level_rule_says(TX):
    for w, h in SIZES + ((4096, 1), (1, 4096), (3, 1000)):
        chain = TX.chain(np.zeros((h, w, 3), np.uint8))
        want = [(w, h)]
        while want[-1] != (1, 1):
            want.append((max(1, want[-1][0] >> 1), max(1, want[-1][1] >> 1)))
        assert [(a, b) for a, b, _ in chain] == want and len(want) == 1 + int(np.floor(np.log2(max(w, h))))
    # a constant texture is constant on every level, and alpha is 255
    for lw, lh, words in TX.chain(np.full((129, 257, 3), (3, 200, 77), np.uint8)):
        assert (words == (3 | 200 << 8 | 77 << 16 | 255 << 24)).all()
    # each level is the rounded mean of 2 x 2 blocks (numpy, integers), with the clamp at odd sizes
    rng = np.random.RandomState(620)
    for w, h in ((64, 64), (5, 3), (1, 7), (257, 129)):
        tex = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        chain = TX.chain(tex)
        cur = tex.astype(np.int64)
        for l, (lw, lh, words) in enumerate(chain):
            got = np.stack([(words >> s) & 255 for s in (0, 8, 16)], -1).reshape(lh, lw, 3)
            np.testing.assert_array_equal(got, cur, err_msg="%d x %d level %d" % (w, h, l))
            assert ((words >> 24) == 255).all()
            ch, cw = cur.shape[:2]
            ys, xs = np.arange(max(1, ch >> 1)), np.arange(max(1, cw >> 1))
            r0, r1 = np.minimum(2 * ys, ch - 1), np.minimum(2 * ys + 1, ch - 1)
            c0, c1 = np.minimum(2 * xs, cw - 1), np.minimum(2 * xs + 1, cw - 1)
            cur = (cur[r0][:, c0] + cur[r0][:, c1] + cur[r1][:, c0] + cur[r1][:, c1] + 2) >> 2
    # Powers of two: a texel of level l + 1 is the exact mean of its four texels plus a rounding error in (-1/2, 1/2], so a
    # level's channel mean is within l / 2 of level 0's: within 1 up to level 2, whatever the bytes (4 x 4 and below), and
    # within l / 2 on the larger ones
    for w, h in ((2, 2), (4, 2), (4, 4), (64, 64), (16, 128)):
        for _ in range(8):
            tex = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
            mean0 = tex.reshape(-1, 3).mean(0)
            for l, (lw, lh, words) in enumerate(TX.chain(tex)):
                mean = np.stack([(words >> s) & 255 for s in (0, 8, 16)], -1).mean(0)
                if (lw << l, lh << l) == (w, h):  # (a level whose blocks are all whole: not behind a side of 1)
                    assert (np.abs(mean - mean0) <= l / 2.0 + 1e-9).all() and (max(w, h) > 4 or l <= 2), (w, h, l)


def camera(ugrt, W, H, eye=(0.3, -5.0, 0.7), look=(0.0, 0.0, 0.0)):
    cam = ugrt.Camera(45.0, W / H)
    cam.setCameraCenter(*eye)
    cam.setCameraLookAt(*look)
    cam.setCameraUp(0, 0, 1)
    cam.adjustCameraAndPosition()
    return cam.camcoords, cam.direction_table()


def plane_gbuffer(ugrt, TX, W, H, eye, look, corners, uv_corners, kd=(0.5, 1.0, 0.25)):
    """A g-buffer of one textured quad (two triangles) seen from `eye`: every pixel hits it (u, v are not clamped, the quad's
    plane is what counts).  One material, texture 0."""
    cc, nodes = camera(ugrt, W, H, eye, look)
    n = W * H
    col, row = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    dirs = TX.directions(cc[:3], nodes, W, H, 0, col, row)
    return dict(W=W, H=H, N=n, cc=cc, nodes=nodes, cam=_f32(cc[:3]), dirs=dirs.reshape(-1), t=np.ones(n, np.float32),
                ids=np.zeros(n, np.int32), verts=_f32(corners).reshape(-1), faces=_i32([0, 1, 2, 0, 2, 3]),
                uvs=_f32(uv_corners).reshape(-1), uv_faces=_i32([0, 1, 2, 0, 2, 3]), mat_idx=_i32([0, 0]),
                mat_list=_f32([0, 0, 0] + list(kd)), mat_texture=_i32([0]))


def test_the_checker_on_a_wall_and_on_a_floor(ugrt, TX):
    rng = np.random.RandomState(621)
    # a wall seen head-on, 8 x 8 texels over far more pixels: magnification
    tex = rng.randint(0, 256, (8, 8, 3)).astype(np.uint8)
    W = H = 64
    wall = plane_gbuffer(ugrt, TX, W, H, (0.0, -4.0, 0.0), (0.0, 0.0, 0.0), [(-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2)],
                         [(0, 0), (1, 0), (1, 1), (0, 1)])
    kd = wall["mat_list"][3:6].astype(np.float64)
    for aniso in (1, 4, 16):
        const, dbg = TX.albedo(wall, [np.full((8, 8, 3), (10, 100, 250), np.uint8)], aniso, 0)
        assert (dbg[:, 3] == 1).all()
        np.testing.assert_allclose(const.reshape(-1, 3), np.tile(kd * np.float64([10, 100, 250]) / 255, (W * H, 1)), rtol=1e-6)
    out, dbg = TX.albedo(wall, [tex], 8, 0)
    # head-on under magnification: level 0, fraction 0.  The footprint's sides are equal up to their rounding, and the
    # rule -- the smallest N with Lmin * N >= Lmax -- says 2 where the longer one is longer by an ulp: N is 1 or 2
    assert (dbg[:, 0] <= 2).all() and (dbg[:, 0] == 1).any() and (dbg[:, 1] == 0).all() and (dbg[:, 2] == 0).all()
    one, _ = TX.albedo(wall, [tex], 1, 0)
    # (two taps a quarter of the footprint, 1/32 texel, to either side: bytes that differ by at most 255 move by 8 / 255)
    np.testing.assert_allclose(out, one, atol=8.0 / 255)
    # the plane's uv at every pixel in float64: at a texel centre the texel, halfway between two their mean
    o, d = wall["cam"].astype(np.float64), wall["dirs"].reshape(-1, 3).astype(np.float64)
    hit = o + d * (-o[1] / d[:, 1])[:, None]
    u, v = (hit[:, 0] + 2) / 4, (hit[:, 2] + 2) / 4
    x, y = u * 8 - 0.5, v * 8 - 0.5
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = x - x0, y - y0
    t64 = tex.astype(np.float64)
    g = lambda yy, xx: t64[yy % 8, xx % 8]
    want = (g(y0, x0) * (1 - fx)[:, None] + g(y0, x0 + 1) * fx[:, None]) * (1 - fy)[:, None] + \
           (g(y0 + 1, x0) * (1 - fx)[:, None] + g(y0 + 1, x0 + 1) * fx[:, None]) * fy[:, None]
    np.testing.assert_allclose(one.reshape(-1, 3), want * kd / 255, atol=2e-3)  # (one tap: the bilinear value at the centre)
    near = (np.abs(fx) < 0.02) & (np.abs(fy) < 0.02)
    assert near.sum() >= 4 and (np.abs(one.reshape(-1, 3)[near] * 255 / kd - g(y0, x0)[near]) < 8).all()
    # +1 of bias raises every level by exactly one; a floor to the horizon: the level does not fall with distance
    W, H = 32, 64
    tex = rng.randint(0, 256, (256, 256, 3)).astype(np.uint8)
    floor = plane_gbuffer(ugrt, TX, W, H, (0.0, 0.0, 1.0), (0.0, 30.0, -0.4), [(-400, 0, 0), (400, 0, 0), (400, 800, 0), (-400, 800, 0)],
                          [(0, 0), (400, 0), (400, 400), (0, 400)])
    facing = floor["dirs"].reshape(-1, 3)[:, 2] < -0.01  # the rays that go down meet the floor in front of the eye
    floor["t"] = np.where(facing, 1.0, 0.0).astype(np.float32)
    iso, di = TX.albedo(floor, [tex], 1, 0)
    an, da = TX.albedo(floor, [tex], 16, 0)
    up, du = TX.albedo(floor, [tex], 16, 1)
    hitrows = facing.reshape(H, W)
    # lambda = Lmax / N falls back by up to a half wherever N steps up, so the level rises with distance where N stands: with
    # one tap everywhere, and with 16 where N has reached 16
    lev = lambda d: (d[:, 1] + np.frombuffer(d[:, 2].astype(np.int32).tobytes(), np.float32)).reshape(H, W)
    dist = (-1.0 / floor["dirs"].reshape(-1, 3)[:, 2]).reshape(H, W)
    for c in range(W):
        rows = np.flatnonzero(hitrows[:, c])
        order = rows[np.argsort(dist[rows, c])]
        assert len(rows) > 10 and (np.diff(lev(di)[order, c]) >= -1e-6).all(), c
        full = order[da.reshape(H, W, 4)[order, c, 0] == 16]
        assert len(full) > 3 and (np.diff(lev(da)[full, c]) >= -1e-6).all(), c
    f = facing
    assert (di[f, 0] == 1).all() and da[f, 0].max() == 16 and da[f, 0].min() <= 4 and (da[f, 1] <= di[f, 1]).all()
    far = f & (dist.reshape(-1) > np.percentile(dist.reshape(-1)[f], 90))
    assert (da[far, 0] == 16).all()
    last = 8
    inner = f & (da[:, 1] + 1 < last) & (da[:, 1] > 0)
    assert inner.sum() > 50 and (du[inner, 1] == da[inner, 1] + 1).all() and (du[inner, 2] == da[inner, 2]).all() and (du[f, 0] == da[f, 0]).all()
    assert (iso.reshape(-1, 3)[~f] == 0).all() and (an.reshape(-1, 3)[~f] == 0).all() and (up.reshape(-1, 3)[f] > 0).all()


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _ctx(ugrt, rows=None, flags=0):
    return ugrt.Context(GW, GH, light_grid=(16, 16), uniform_dims=(8, 8, 8), rows=rows, flags=flags)


def _levels(ctx, tex, count):
    out = []
    for l in range(count):
        w, h, words = ctx.texture_get_level(tex, l)
        out.append((w, h, words.cpu().numpy().view(np.uint32).copy()))
    return out


@pytest.mark.gpu
def test_every_level_of_five_textures_in_one_atlas(ugrt, TX, torch):
    texs = textures()
    ctx = _ctx(ugrt)
    assert ctx.get_state("texture_builds") == 0 and ctx.get_state("texture_count") == 0
    for n_set, subset in enumerate((texs, [texs[4], texs[2]], texs[::-1], [texs[1]]), 1):
        ctx.texture_set(subset)
        ctx.synchronize()
        assert ctx.get_state("texture_builds") == n_set and ctx.get_state("texture_count") == len(subset)
        for i, tex in enumerate(subset):
            want = TX.chain(tex)
            got = _levels(ctx, i, len(want))
            for l, ((ww, wh, wwords), (gw, gh, gwords)) in enumerate(zip(want, got)):
                assert (ww, wh) == (gw, gh), (n_set, i, l)
                np.testing.assert_array_equal(gwords, wwords, err_msg="set %d, texture %d, level %d" % (n_set, i, l))
            with pytest.raises(ugrt.UgrtError):
                ctx.texture_get_level(i, len(want))
        with pytest.raises(ugrt.UgrtError):
            ctx.texture_get_level(len(subset), 0)
    ctx.texture_set([])
    assert ctx.get_state("texture_builds") == 4 and ctx.get_state("texture_count") == 0
    with pytest.raises(ugrt.UgrtError):
        ctx.texture_get_level(0, 0)
    # the drop freed the device arrays: an atlas after it is built into new ones
    ctx.texture_set([texs[2], texs[4]])
    ctx.synchronize()
    for i, tex in enumerate((texs[2], texs[4])):
        want = TX.chain(tex)
        for (ww, wh, wwords), (gw, gh, gwords) in zip(want, _levels(ctx, i, len(want))):
            assert (ww, wh) == (gw, gh)
            np.testing.assert_array_equal(gwords, wwords)
    assert ctx.get_state("texture_builds") == 5 and ctx.get_state("texture_count") == 2


_G = {}


def gbuffer(ugrt, TX, seed=622):
    """A synthetic g-buffer of 64 x 40 pixels over 200 seeded triangles and special ones behind them; computed once and
    shared: nobody writes to it.  Materials: 0 and 6 untextured, 1..5 texture 0..4; mat_idx also holds -1 and 7."""
    if _G:
        return _G
    rng = np.random.RandomState(seed)
    W, H, F, V, T = GW, GH, 200, 150, 120
    n = W * H
    cc, nodes = camera(ugrt, W, H)
    eye = _f32(cc[:3])
    col, row = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    dirs = TX.directions(eye, nodes, W, H, 0, col, row)
    dirx = TX.directions(eye, nodes, W, H, 0, col + 1, row)
    verts = list(rng.uniform(-2, 2, (V, 3)) * rng.choice([0.05, 1.0, 30.0], (V, 1)))
    faces = [list(rng.permutation(V)[:3]) for _ in range(F)]
    uvs = list(rng.uniform(-3, 3, (T, 2)) * rng.choice([0.01, 1.0, 1.0, 40.0], (T, 1)))
    uv_faces = [list(rng.randint(0, T, 3)) for _ in range(F)]
    ids = rng.randint(0, F, n).astype(np.int32)

    def add_face(vs, ts):
        """a face of new vertices (positions or indices) and new uvs (pairs or indices); returns its id"""
        f = []
        for v in vs:
            if np.ndim(v) == 0:
                f.append(int(v))
            else:
                verts.append(np.asarray(v, np.float64))
                f.append(len(verts) - 1)
        u = []
        for t in ts:
            if np.ndim(t) == 0:
                u.append(int(t))
            else:
                uvs.append(np.asarray(t, np.float64))
                u.append(len(uvs) - 1)
        faces.append(f)
        uv_faces.append(u)
        return len(faces) - 1

    tri = lambda: [rng.uniform(-2, 2, 3) for _ in range(3)]
    special = {}
    # constant uvs: a' that rounds to exactly 1.0; texel centres and edges of the 5 x 3 texture to the ulp and beside; Lx == Ly == 0
    one = np.float32(1.0)
    consts = [(-1e-9, -1e-9), (-1e-9, 0.5), (1.0, 1.0), (0.0, 0.0), (-0.0, -0.0)]
    for k in range(5):
        for j in range(3):
            for base in ((k + 0.5) / 5, k / 5.0):
                b = np.float32(base)
                for a in (b, np.nextafter(b, one + 1), np.nextafter(b, -one)):
                    consts.append((float(a), float(np.float32((j + 0.5) / 3))))
                    consts.append((float(a), float(np.float32(j / 3.0))))
    special["const"] = [add_face(tri(), [c, c, c]) for c in consts]
    # degenerate triangles, uv indices of -1 and num_uvs (patched below), huge and non-finite uvs
    a, b = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
    special["degenerate"] = [add_face([a, a, b], [0, 1, 2]), add_face([a, a, a], [3, 4, 5]), add_face([a, b, 2 * b - a], [6, 7, 8])]
    special["bad_uv"] = [add_face(tri(), [-1, 1, 2]), add_face(tri(), [0, 1, -7]), add_face(tri(), [0, 10 ** 6, 2]), add_face(tri(), [0, 1, 2])]
    special["huge_uv"] = [add_face(tri(), [(0, 0), (3e38, 0), (0, 0)]), add_face(tri(), [(1e30, 1), (1e30, 2), (1e30, 3)]),
                          add_face(tri(), [(0, 0), (1e34, -1e34), (1, 1)]), add_face(tri(), [(np.inf, 0), (0, 0), (0, 1)]),
                          add_face(tri(), [(np.nan, 0), (0, 0), (0, 1)]), add_face(tri(), [(0, 0), (1e6, 0), (0, 1e6)]),
                          add_face(tri(), [(0, 0), (2e4, 0), (0, 3e4)])]
    pool = np.concatenate([np.asarray(v) for v in special.values()])
    pick = rng.choice(n, n // 3, replace=False)
    ids[pick] = pool[rng.randint(0, len(pool), len(pick))]
    # edge-on to the eye: the stored direction is the triangle's second edge (the determinant is exactly 0)
    edge_on = np.arange(n) % 8 == 3
    # edge-on to the (col + 1) ray only: v0 = the origin and v2 = twice that ray's direction, so that e2 is that exactly and
    # CROSS(d, e2) is exactly 0 for the neighbour's d
    edge_x = np.flatnonzero(np.arange(n) % 64 == 21)
    for p in edge_x:
        ids[p] = add_face([np.zeros(3), rng.uniform(-2, 2, 3), 2.0 * dirx[p].astype(np.float64)], list(rng.randint(0, T, 3)))
    edge_x_faces = ids[edge_x].copy()
    verts = np.asarray(verts, np.float64).astype(np.float32)
    faces = np.asarray(faces, np.int32)
    uvs = np.asarray(uvs, np.float64).astype(np.float32)
    uv_faces = np.asarray(uv_faces, np.int32)
    uv_faces[special["bad_uv"][3], 1] = len(uvs)  # == num_uvs
    dirs = dirs.copy()
    hit_ids = np.maximum(ids, 0)
    dirs[edge_on] = (verts[faces[hit_ids, 2]] - verts[faces[hit_ids, 0]])[edge_on]
    cam = eye.copy()
    ids[rng.choice(n, n // 12, replace=False)] = rng.choice([-1, -2, -2 ** 31], n // 12)
    t = rng.uniform(0.5, 9.0, n).astype(np.float32)
    odd = np.float32([np.nan, 0.0, -0.0, 1e-42, np.inf, -3.0, -np.inf, -1e-42])
    pick = rng.choice(n, n // 6, replace=False)
    t[pick] = odd[rng.randint(0, len(odd), len(pick))]
    M = 7
    mat_idx = rng.randint(1, 6, len(faces)).astype(np.int32)
    other = rng.choice(len(faces), len(faces) // 5, replace=False)
    mat_idx[other] = rng.choice([-1, 7, 0, 6, -2 ** 31, 2 ** 31 - 1], len(other))
    mat_idx[special["const"]] = 3  # the 5 x 3 texture
    mat_idx[edge_x_faces] = 5
    mat_idx[special["huge_uv"]] = [4, 5, 4, 5, 4, 5, 4]
    mat_list = rng.uniform(0, 1, 6 * M).astype(np.float32)
    mat_texture = _i32([-1, 0, 1, 2, 3, 4, -5])
    normal = rng.uniform(-1, 1, (n, 3))
    normal = (normal / np.sqrt((normal * normal).sum(1))[:, None]).astype(np.float32)
    _G.update(W=W, H=H, N=n, cc=cc, nodes=nodes, cam=cam, dirs=dirs.reshape(-1), t=t, ids=ids, verts=verts.reshape(-1), faces=faces.reshape(-1),
              uvs=uvs.reshape(-1), uv_faces=uv_faces.reshape(-1), mat_idx=mat_idx, mat_list=mat_list, mat_texture=mat_texture,
              edge_on=edge_on, edge_x=edge_x, special=special, normal=normal.reshape(-1), M=M)
    return _G


DEVICE_KEYS = ("t", "dirs", "ids", "cam", "verts", "faces", "uvs", "uv_faces", "mat_idx", "mat_list", "mat_texture")


def _device_albedo(torch, ctx, g, d, max_aniso, lod_bias, fill=7.0):
    out = torch.full((3 * g["N"],), fill, dtype=torch.float32, device=ctx.device)
    ctx.texture_albedo(d["t"], d["dirs"], d["ids"], d["cam"], d["verts"], d["faces"], d["uvs"], len(g["uvs"]) // 2, d["uv_faces"],
                       d["mat_idx"], d["mat_list"], g["M"], d["mat_texture"], g["mat_texture"], max_aniso, lod_bias, out)
    ctx.synchronize()
    return out


def test_the_synthetic_gbuffer_reaches_every_branch(ugrt, TX):
    """(CPU) what the GPU test below compares is worth comparing: the checker's view of the g-buffer."""
    g = gbuffer(ugrt, TX)
    texs = textures()
    out, dbg = TX.albedo(g, texs, 16, 0)
    n = g["N"]
    o3 = out.reshape(-1, 3)
    hit = (g["ids"] >= 0) & (g["t"] > 0)
    m = np.where(hit, g["mat_idx"][np.maximum(g["ids"], 0)], -1)
    inrange = hit & (m >= 0) & (m < g["M"])
    assert 300 < (~hit).sum() and (o3[~inrange] == 0).all() and not np.signbit(o3[~inrange]).any()
    filtered = dbg[:, 3] == 1
    kd = g["mat_list"].reshape(-1, 6)[np.clip(m, 0, 6), 3:]
    plain = inrange & ~filtered
    assert np.array_equal(bits(o3[plain]), bits(kd[plain])) and plain.sum() > 200
    assert not filtered[inrange & g["edge_on"]].any() and (inrange & g["edge_on"]).sum() > 50
    assert not filtered[inrange & np.isin(m, (0, 6))].any()
    uvf = g["uv_faces"].reshape(-1, 3)
    assert not filtered[np.isin(g["ids"], g["special"]["bad_uv"])].any()
    assert set(np.unique(dbg[filtered, 0])) == set(range(1, 17)), np.unique(dbg[filtered, 0])
    big = filtered & (m == 5)  # 257 x 129: nine levels
    assert set(np.unique(dbg[big, 1])) == set(range(9)), np.unique(dbg[big, 1])
    assert set(np.unique(m[filtered])) == {1, 2, 3, 4, 5}
    ex = np.zeros(n, bool)
    ex[g["edge_x"]] = True
    fall = filtered & ex & (m == 5)
    assert fall.sum() >= 3 and (dbg[fall, 0] == 1).all() and (dbg[fall, 1] == 8).all()   # a neighbour's determinant failed
    huge = filtered & np.isin(g["ids"], g["special"]["huge_uv"]) & (m >= 4)
    assert huge.sum() >= 3 and ((dbg[huge, 0] == 1) & (dbg[huge, 1] == np.where(m[huge] == 4, 6, 8))).sum() >= 3
    const = filtered & np.isin(g["ids"], g["special"]["const"])
    # constant uvs: the footprint is 0 or the mix's rounding (any N, taps a rounding apart), level 0; Lx == Ly == 0 is there
    assert const.sum() > 100 and (dbg[const, 1] == 0).all() and (dbg[const, 2] == 0).all() and (dbg[const, 0] == 1).any()
    assert np.isfinite(o3[filtered & ~np.isin(g["ids"], g["special"]["huge_uv"])]).all()
    # the other parameters move the taps and the levels
    for aniso, bias in ((1, 0), (2, -16), (8, 3), (16, 16)):
        o2, d2 = TX.albedo(g, texs, aniso, bias)
        assert np.array_equal(d2[:, 3], dbg[:, 3]) and d2[filtered, 0].max() == aniso
        if bias == -16:
            assert (d2[filtered & ~ex & ~huge, 1] == 0).sum() > 1000
        if bias == 16:
            assert (d2[big & (dbg[:, 0] > 1), 1] == 8).all()


@pytest.mark.gpu
@pytest.mark.parametrize("max_aniso,lod_bias,strict", [(1, 0, 0), (2, -16, 0), (8, 3, 0), (16, 16, 0), (16, 0, 0), (16, 0, 1), (8, -2, 1)])
def test_the_albedo_on_a_synthetic_gbuffer(ugrt, TX, torch, max_aniso, lod_bias, strict):
    g = gbuffer(ugrt, TX)
    texs = textures()
    want, _ = TX.albedo(g, texs, max_aniso, lod_bias, strict)
    ctx = _ctx(ugrt, flags=ugrt.FLAG_STRICT_TEXTURE if strict else 0)
    ctx.upload_camera(g["cc"])
    ctx.texture_set(texs)
    d = {k: ctx.upload(g[k]) for k in DEVICE_KEYS}
    got = _device_albedo(torch, ctx, g, d, max_aniso, lod_bias)
    assert_same(got.cpu().numpy(), want, "aniso %d, bias %d" % (max_aniso, lod_bias))
    for k in DEVICE_KEYS:  # the inputs are only read
        assert np.array_equal(d[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(g[k]).view(np.uint32)), k
    if strict or max_aniso != 16:
        return
    # a band: the rows outside keep the fill
    band = _ctx(ugrt, rows=(1, 4))
    p0, m = 8 * GW, 24 * GW
    assert (band.p0, band.npix) == (p0, m)
    band.upload_camera(g["cc"])
    band.texture_set(texs)
    db = {k: band.upload(g[k]) for k in DEVICE_KEYS}
    got = _device_albedo(torch, band, g, db, max_aniso, lod_bias).cpu().numpy()
    banded, _ = TX.albedo(g, texs, max_aniso, lod_bias, 0, p0, m)
    assert_same(got, banded, "a band")
    assert (got[:3 * p0] == 7.0).all() and (got[3 * (p0 + m):] == 7.0).all()
    np.testing.assert_array_equal(bits(banded[3 * p0:3 * (p0 + m)]), bits(want[3 * p0:3 * (p0 + m)]))
    # fewer textures in a second atlas: the materials that named the others are checked, the rest filters from new offsets
    ctx.texture_set([texs[4], texs[2]])
    g2 = dict(g, mat_texture=_i32([-1, 0, 1, 0, 1, -1, -5]))
    d2 = dict(d, mat_texture=ctx.upload(g2["mat_texture"]))
    want2, _ = TX.albedo(g2, [texs[4], texs[2]], 4, 0)
    assert_same(_device_albedo(torch, ctx, g2, d2, 4, 0).cpu().numpy(), want2, "the second atlas")


def _oracle_images(O, LTref, g, albedo, lights, flags, spot=False):
    """The image of the oracle's shading call (one light) or of the lights checker's, given one material per pixel whose
    Kd is the pixel's albedo: mat_idx = arange, a pixel whose material is out of range keeps an id out of range."""
    n = g["N"]
    tri = g["ids"]
    m = np.where(tri >= 0, g["mat_idx"][np.maximum(tri, 0)], tri)
    ok = (m >= 0) & (m < g["M"])
    ids = np.where(ok, np.arange(n), -1).astype(np.int32)
    mat_list = np.zeros((n, 6), np.float32)
    mat_list[:, 3:] = albedo.reshape(-1, 3)
    if lights is None:
        img = np.zeros(3 * n, np.uint8)
        O.shade(g["cc"], g["light"], img, _f32(g["normal"]), _f32(g["t"]), _f32(g["dirs"]), ids, g["cam"], np.arange(n), mat_list, 0, n,
                spot=spot)
        return img
    return LTref.shade_lights(g["cc"], g["normal"], g["t"], g["dirs"], ids, g["cam"], np.arange(n), mat_list, lights, flags, 0, n, n)[0]


@pytest.mark.gpu
def test_the_shading_calls_read_the_albedo_in_the_place_of_kd(ugrt, TX, O, LT, torch):
    g = dict(gbuffer(ugrt, TX))
    rng = np.random.RandomState(623)
    n = g["N"]
    g["light"] = np.float32([1.5, -3.0, 4.0])
    albedo, _ = TX.albedo(g, textures(), 8, 0)
    m = np.where(g["ids"] >= 0, g["mat_idx"][np.maximum(g["ids"], 0)], g["ids"])
    kd = g["mat_list"].reshape(-1, 6)[np.clip(m, 0, g["M"] - 1), 3:].reshape(-1).astype(np.float32)
    ctx = _ctx(ugrt)
    ctx.upload_camera(g["cc"])
    ctx.set_light_position(g["light"])
    d = {k: ctx.upload(g[k]) for k in ("normal", "t", "dirs", "cam", "mat_idx", "mat_list")}
    want_ids = m.astype(np.int32)

    def run(call, alb, *extra):
        img = torch.full((3 * n,), 0xA5, dtype=torch.uint8, device=ctx.device)
        ids = ctx.upload(g["ids"])
        args = [img, d["normal"], d["t"], d["dirs"], ids, d["cam"], d["mat_idx"], d["mat_list"], g["M"]] + list(extra)
        call(*(args + ([] if alb is None else [ctx.upload(alb)])))
        ctx.synchronize()
        np.testing.assert_array_equal(ids.cpu().numpy(), want_ids)
        return img.cpu().numpy()

    got = run(ctx.texture_shade, albedo)
    np.testing.assert_array_equal(got, _oracle_images(O, LT, g, albedo, None, None))
    assert (got != run(ctx.shade_simple, None)).mean() > 0.1
    np.testing.assert_array_equal(run(ctx.texture_shade, kd), run(ctx.shade_simple, None))
    got = run(ctx.texture_shade_spotlight, albedo)
    np.testing.assert_array_equal(got, _oracle_images(O, LT, g, albedo, None, None, spot=True))
    assert (got != run(ctx.shade_spotlight, None)).mean() > 0.1
    np.testing.assert_array_equal(run(ctx.texture_shade_spotlight, kd), run(ctx.shade_spotlight, None))
    for L in (1, 3, 8):
        lights = rng.uniform(-4, 4, (L, 3)).astype(np.float32)
        for flags in (None, (rng.uniform(size=(L, n)) < 0.3).astype(np.int32)):
            dflags = None if flags is None else ctx.upload(flags.reshape(-1))
            got = run(ctx.texture_shade_lights, albedo, lights, dflags)
            np.testing.assert_array_equal(got, _oracle_images(O, LT, g, albedo, lights, flags), err_msg="%d lights" % L)
            np.testing.assert_array_equal(run(ctx.texture_shade_lights, kd, lights, dflags), run(ctx.shade_lights, None, lights, dflags))


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing(ugrt, TX, torch):
    g = gbuffer(ugrt, TX)
    texs = textures()
    n = g["N"]
    ctx = _ctx(ugrt)
    ctx.upload_camera(g["cc"])
    d = {k: ctx.upload(g[k]) for k in DEVICE_KEYS}
    d["normal"] = ctx.upload(g["normal"])
    out = torch.full((3 * n,), 7.0, dtype=torch.float32, device=ctx.device)
    img = torch.full((3 * n,), 0xA5, dtype=torch.uint8, device=ctx.device)
    ids = ctx.upload(g["ids"])
    ctx.prof_enable(True)

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    def albedo_args(**kw):
        a = dict(t=d["t"], dirs=d["dirs"], ids=d["ids"], cam=d["cam"], verts=d["verts"], faces=d["faces"], uvs=d["uvs"],
                 num_uvs=len(g["uvs"]) // 2, uv_faces=d["uv_faces"], mat_idx=d["mat_idx"], mat_list=d["mat_list"], M=g["M"],
                 mat_texture=d["mat_texture"], host=g["mat_texture"], aniso=8, bias=0, out=out)
        a.update(kw)
        return list(a.values())

    # no atlas, and a material names a texture
    fails(ctx.texture_albedo, albedo_args(), b"the atlas holds 0")
    for bad, word in (([np.zeros((0, 4, 3), np.uint8)], b"outside 1.."), ([np.zeros((1, 4097, 3), np.uint8)], b"outside 1.."),
                      ([np.zeros((2, 2, 3), np.uint8)] * 65, b"not in 0..64")):
        fails(ctx.texture_set, (bad,), word)
    assert ctx.get_state("texture_builds") == 0 and ctx.get_state("texture_count") == 0
    counts = ctx.prof_get()
    assert counts["build_fill"][1] == 0 and counts["shade"][1] == 0  # nothing was launched
    ctx.texture_set(texs[:3])
    fails(ctx.texture_albedo, albedo_args(), b"the atlas holds 3")
    ctx.texture_set(texs)
    fills = ctx.prof_get()["build_fill"][1]
    for bad in ([np.zeros((0, 4, 3), np.uint8)], [np.zeros((2, 2, 3), np.uint8)] * 65):  # the atlas of the call before stands
        fails(ctx.texture_set, (bad,), b"texture_set")
    assert ctx.prof_get()["build_fill"][1] == fills and ctx.get_state("texture_count") == 5 and ctx.get_state("texture_builds") == 2
    for key in ("t", "dirs", "ids", "cam", "verts", "faces", "uvs", "uv_faces", "mat_idx", "mat_list", "mat_texture", "out"):
        fails(ctx.texture_albedo, albedo_args(**{key: None}), b"null")
    for kw, word in ((dict(aniso=0), b"max_aniso"), (dict(aniso=17), b"max_aniso"), (dict(bias=-17), b"lod_bias"), (dict(bias=17), b"lod_bias"),
                     (dict(num_uvs=-1), b"negative"), (dict(M=-1), b"negative"), (dict(host=_i32([-1, 0, 1, 2, 3, 5, -5])), b"names texture 5")):
        fails(ctx.texture_albedo, albedo_args(**kw), word)
    alb = torch.zeros(3 * n, dtype=torch.float32, device=ctx.device)
    base = [img, d["normal"], d["t"], d["dirs"], ids, d["cam"], d["mat_idx"], d["mat_list"], g["M"]]
    fails(ctx.texture_shade, base + [None], b"null")
    fails(ctx.texture_shade_spotlight, base + [None], b"null")
    fails(ctx.texture_shade_spotlight, [None] + base[1:] + [alb], b"null")
    for h in range(8):
        a = list(base) + [alb]
        a[h] = None
        fails(ctx.texture_shade, a, b"null")
    lights = np.float32([[1, 2, 3]])
    fails(ctx.texture_shade_lights, base + [lights, None, None], b"null")
    fails(ctx.texture_shade_lights, base + [np.zeros((9, 3), np.float32), None, alb], b"num_lights")
    fails(ctx.texture_shade_lights, base + [None, None, alb], b"null")
    ctx.synchronize()
    assert (out == 7.0).all() and (img == 0xA5).all() and np.array_equal(ids.cpu().numpy(), g["ids"])
    assert ctx.prof_get()["shade"][1] == 0  # no launch in the shading stage
    # the context is usable afterwards
    want, _ = TX.albedo(g, texs, 8, 0)
    assert_same(_device_albedo(torch, ctx, g, d, 8, 0).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------ the renderer

import copy  # noqa: E402

import frame_ref as FR  # noqa: E402
import test_area_light as TA  # noqa: E402
import test_lights as TL  # noqa: E402
import test_reflect_lights as RLT  # noqa: E402
import test_smooth as TS  # noqa: E402
import test_temporal as TT  # noqa: E402
from test_ambient import AO  # noqa: F401,E402  (fixtures of K)
from test_ambient_sets import ASR  # noqa: F401,E402
from test_antialias import AA  # noqa: F401,E402
from test_area_light import AR  # noqa: F401,E402
from test_filter_visibility import SR  # noqa: F401,E402
from test_frame_matrix import K  # noqa: F401,E402
from test_glossy import GL  # noqa: F401,E402
from test_indirect import IR  # noqa: F401,E402
from test_reflect_lights import RL  # noqa: F401,E402
from test_reflect_shadows import REFS  # noqa: F401,E402
from test_refract import RF  # noqa: F401,E402
from test_smooth import SM  # noqa: F401,E402
from test_temporal import TR  # noqa: F401,E402

LG, UD = RD.LG, RD.UD
FW = FH = 128


def _fake(ugrt):
    r = TT._fake(ugrt)
    r.__dict__.update(albedo="albedo", snormal="snormal", corner_normals="cn",
                      _tex=dict(uvs="uv", num_uvs=5, uv_faces="uvf", mat_texture="mt", mat_texture_host="mth"))
    r._texture_stage = lambda: r.ctx.calls.append(("texture_stage",))
    r._smooth_stage = lambda cos: r.ctx.calls.append(("smooth_stage", cos))
    return r


def test_textures_are_checked_before_anything_runs(ugrt):
    chk = RLT._rmod(ugrt).check_textures
    assert chk(False) is None and chk(np.bool_(False), 8, 0, reflect=True, gi=4, two_streams=True) is None
    assert chk(True) == (8, 0) and chk(True, 1, -16) == (1, -16) and chk(True, np.int32(16), 16) == (16, 16)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError):
            chk(bad)
    for bad in (0, 17, 2.0, True, "8", None):
        with pytest.raises(ValueError):
            chk(True, bad)
    for bad in (-17, 17, 0.0, True, None):
        with pytest.raises(ValueError):
            chk(True, 8, bad)
    for kw in (dict(texture_aniso=4), dict(texture_bias=1)):  # a value away from its default needs textures
        with pytest.raises(ValueError):
            chk(False, **kw)
    assert chk(True, frame_cnt=2) == (8, 0)
    excluded = (dict(reflect=True), dict(refract=True), dict(fresnel=True), dict(glossy=4), dict(gi=8), dict(aa=4), dict(dof=4),
                dict(reflect_lights=True), dict(two_streams=True))
    for kw in excluded:
        with pytest.raises(ValueError):
            chk(True, **kw)
    s = RD.scene(ugrt, "hall")
    single, multi = TL.setup_for(ugrt, s), TL.setup_for(ugrt, s, TL.lights_for(s, 2))
    illegal = (dict(reflect=True), dict(reflect=True, refract=True), dict(reflect=True, refract=True, fresnel=True), dict(glossy=4),
               dict(gi=8), dict(aa=4), dict(dof=4, dof_aperture=0.1), dict(texture_aniso=0), dict(texture_bias=17))
    for kw in illegal:
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(single, textures=True, **kw)
        assert r.ctx.calls == [] and r.cleared == [], kw
    for kw in (dict(texture_aniso=4), dict(texture_bias=-1), dict(textures=1)):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(single, **kw)
        assert r.ctx.calls == []
    r = _fake(ugrt)
    with pytest.raises(ValueError):
        r.display(multi, textures=True, reflect=True, reflect_lights=True)
    assert r.ctx.calls == []
    for kw in (dict(), dict(shadows=False), dict(ao=4, ao_radius=1.0)):  # the two-stream renderer
        r = _fake(ugrt)
        r.aux = object()
        with pytest.raises(ValueError):
            r.display(single, textures=True, **kw)
        assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    for kw in (dict(textures=True), dict(textures=True, reflect=False), dict(texture_aniso=4), dict(texture_bias=2)):
        with pytest.raises(ValueError):
            br.display(single, **kw)


def test_a_textured_frame_enqueues_one_pass_behind_the_camera_pass_and_the_default_frame_nothing(ugrt):
    s = RD.scene(ugrt, "hall")
    single, multi = TL.setup_for(ugrt, s), TL.setup_for(ugrt, s, TL.lights_for(s, 2))
    names = TA._names
    frames = ((single, dict(), "shade_simple", "texture_shade"), (single, dict(frame_cnt=2), "shade_spotlight", "texture_shade_spotlight"),
              (single, dict(shadows=False), "shade_simple", "texture_shade"),
              (multi, dict(), "shade_lights", "texture_shade_lights"), (single, dict(ao=4, ao_radius=1.0), "shade_simple", "texture_shade"),
              (single, dict(area=5, area_radius=0.5), "shade_simple", "texture_shade"),
              (single, dict(ao=4, ao_radius=1.0, temporal=4), "shade_simple", "texture_shade"),
              (single, dict(smooth=True), "shade_simple", "texture_shade"), (multi, dict(ao=4, ao_radius=1.0), "shade_lights", "texture_shade_lights"))
    for setup, kw, shade, shade_tex in frames:
        a, b, c = _fake(ugrt), _fake(ugrt), _fake(ugrt)
        a.display(setup, **kw)
        b.display(setup, textures=False, texture_aniso=8, texture_bias=0, **kw)
        assert names(a) == names(b) and "texture_albedo" not in names(a) and "texture_stage" not in names(a)
        c.display(setup, textures=True, texture_aniso=4, texture_bias=-1, **kw)
        at = names(c).index("texture_stage")
        assert names(c)[at - 1] == "trace_primary" and names(c)[at + 1] == "texture_albedo" and names(c)[at + 2] == "upload_camera", kw
        assert c.ctx.calls[at + 1] == ("texture_albedo", "t", "d", "ids", "cam", "v", "f", "uv", 5, "uvf", "mi", "ml", c.num_materials,
                                       "mt", "mth", 4, -1, "albedo"), c.ctx.calls[at + 1]
        rest = names(c)[:at] + names(c)[at + 2:]
        assert [shade if x == shade_tex else x for x in rest] == names(a), kw
        sh_c, sh_a = c.ctx.calls[names(c).index(shade_tex)], a.ctx.calls[names(a).index(shade)]
        assert sh_c[-1] == "albedo" and len(sh_c) == len(sh_a) + 1
        assert [x for x in sh_c[1:-1] if isinstance(x, (str, int, float))] == [x for x in sh_a[1:] if isinstance(x, (str, int, float))]
        # nothing else reads the new buffer
        assert sum("albedo" in [x for x in call if isinstance(x, str)] for call in c.ctx.calls) == 2
        c = _fake(ugrt)
        c.display(setup, textures=True, shade=False, **kw)
        assert names(c) == names(b)[:len(names(c))] and "texture_albedo" not in names(c)


def test_write_scene_keeps_its_bytes_and_round_trips_the_textured_scene(ugrt, tmp_path):
    import hashlib

    c = ugrt.scenes.cornell(str(tmp_path / "c"))
    got = {e: hashlib.md5(open(c[e], "rb").read()).hexdigest() for e in ("obj", "mtl", "mat")}
    # the files the scene writer gave before it knew uvs and textures (md5 of cornell.obj / .mtl / .mat)
    assert {k: v[:8] for k, v in got.items()} == {"obj": "613d0026", "mtl": "a2820e77", "mat": "6a8337be"}
    assert sorted(os.listdir(tmp_path / "c")) == ["cornell.mat", "cornell.mtl", "cornell.obj"]
    s = ugrt.scenes.textured(str(tmp_path / "t"))
    m = ugrt.Model()
    m.some_material(s["mat"])
    m.load_model(s["obj"])
    want = np.float32([float("%.6f" % x) for x in s["uvs"].reshape(-1)])
    np.testing.assert_array_equal(m.h_uvlist, want)
    np.testing.assert_array_equal(m.h_uvfacelist.reshape(-1, 3), s["uv_faces"])
    assert m.h_texturelist == ["floor_checker.ppm", "wall_checker.ppm", "", "box_stripes.ppm"] and m.texture_dir == str(tmp_path / "t") + "/"
    np.testing.assert_array_equal(m.h_facelist.reshape(-1, 3), s["faces"])
    np.testing.assert_array_equal(m.h_materiallist_index, s["matidx"])
    for k, name in enumerate(m.h_texturelist):
        if name:
            np.testing.assert_array_equal(ugrt.read_ppm(m.texture_dir + name), s["textures"][s["mat_texture"][k]])
    assert (s["uv_faces"][s["matidx"] == 2] == -1).all() and (s["uv_faces"][s["matidx"] != 2] >= 0).all()
    # planar_uvs: the dominant axis is dropped; the procedural textures
    uv, uf = ugrt.scenes.planar_uvs(np.float32([[0, 0, 5], [2, 0, 5], [0, 3, 5], [1, 0, 0], [1, 2, 0], [1, 0, 4]]), [[0, 1, 2], [3, 4, 5]], 0.5)
    np.testing.assert_array_equal(uv, np.float32([[0, 0], [1, 0], [0, 1.5], [0, 0], [1, 0], [0, 2]]))
    np.testing.assert_array_equal(uf, [[0, 1, 2], [3, 4, 5]])
    ch = ugrt.scenes.checker_texture(8, 4)
    assert ch.shape == (8, 8, 3) and ch.dtype == np.uint8 and (ch[0, 0] == ch[1, 1]).all() and (ch[0, 0] != ch[0, 2]).any() and (ch[0, 0] == ch[2, 2]).all()
    st = ugrt.scenes.stripes_texture(16, 4)
    assert st.shape == (16, 16, 3) and (st[0] == st[7]).all() and (st[0, 0] != st[0, 4]).any() and (st[0, 0] == st[0, 3]).all()


_TF = {}


def tframes(K):  # noqa: F811
    if "F" not in _TF:
        s = dict(K.ugrt.scenes.textured(scale=0.1))
        s["vertex_key"] = K.ugrt.scenes.weld(s["verts"], 1e-5)
        _TF["F"] = FR.Frames(K, s, FW, FH)
    return _TF["F"]


def frame_gbuffer(F, setup):
    """The frame's primary hits and its scene as the checker's calls take them."""
    P, s = FR.primary(F, setup), F.scene
    pr = P["pr"]
    cam = F.K.rmod.make_camera(setup.camera, setup.fovy, float(np.float32(F.W) / np.float32(F.H)))
    return dict(W=F.W, H=F.H, N=F.N, cc=np.asarray(cam.camcoords, np.float32), nodes=cam.direction_table(), cam=_f32(P["cam_pos"]),
                dirs=pr["dir"], t=pr["t"], ids=pr["id"], verts=F.verts, faces=F.faces, uvs=_f32(s["uvs"]).reshape(-1),
                uv_faces=_i32(s["uv_faces"]).reshape(-1), mat_idx=_i32(s["matidx"]), mat_list=_f32(s["mat_list"]).reshape(-1),
                mat_texture=_i32(s["mat_texture"]))


def frame_albedo(TX, F, setup, aniso, bias):
    """The checker's albedo of the frame's primary hits."""
    return F.once(("albedo", FR._setup_key(setup), aniso, bias),
                  lambda: TX.albedo(frame_gbuffer(F, setup), F.scene["textures"], aniso, bias))


def textured_frames(F, setup, albedo, lights, shadows):
    """F with the albedo in the place of the materials' Kd in frame_ref's shading call: a copy that answers the "shaded" key
    with the oracle's shading given one material per pixel, and shares every other cache entry."""
    K, s, N = F.K, F.scene, F.N

    def shaded(spot):
        P = FR.primary(F2, setup)
        pr = P["pr"]
        tri = pr["id"]
        m = np.where(tri >= 0, _i32(s["matidx"])[np.maximum(tri, 0)], tri).astype(np.int32)
        ok = (m >= 0) & (m < len(s["mat_list"]))
        ids = np.where(ok, np.arange(N), -1).astype(np.int32)
        mats = np.zeros((N, 6), np.float32)
        mats[:, 3:] = albedo.reshape(-1, 3)
        if lights:
            per = P["lights"]
            flags = np.stack([lt["flags"] for lt in per]) if shadows else None
            img, _ = K.LT.shade_lights(per[-1]["cc"], pr["normal"], pr["t"], pr["dir"], ids, P["cam_pos"], np.arange(N), mats,
                                       [lt["pos"] for lt in per], flags, 0, N, N)
        else:
            img = np.zeros(3 * N, np.uint8)
            K.O.shade(P["lcam"].cc, setup.shading_light, img, pr["normal"], pr["t"], pr["dir"], ids, P["cam_pos"], np.arange(N), mats, 0, N,
                      spot=spot)
        return img, m

    def once(self, key, make):
        return shaded(len(key) > 2 and bool(key[2])) if key[0] == "shaded" else FR.Frames.once(self, key, make)

    F2 = copy.copy(F)
    F2.__class__ = type("TexturedFrames", (FR.Frames,), {"once": once})
    return F2


def _make(F):
    u, s = F.K.ugrt, F.scene
    ctx = u.Context(F.W, F.H, light_grid=LG, flags=u.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
    return ctx, u.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], vertex_key=s["vertex_key"],
                           uvs=s["uvs"], uv_faces=s["uv_faces"], textures=s["textures"], mat_texture=s["mat_texture"])


@pytest.mark.gpu
def test_textured_frames_equal_the_cpu_frames(ugrt, TX, SM, K, torch):  # noqa: F811
    """display(textures=True) at 128 x 128 on scenes.textured(): plain, frame_cnt=2, shadows=False, three lights, and with smooth, ao and
    area: everything the frame leaves behind is frame_ref's with the checker's albedo in the shading call, and everything
    but the image is the frame's without textures."""
    F = tframes(K)
    s = F.scene
    single = F.setup
    multi = ugrt.FrameSetup.from_scene(s, lights=TL.lights_for(s, 3))
    r_ao, r_area = float(np.float32(0.02 * F.extent)), float(np.float32(0.01 * F.extent))
    todo = (("plain", dict(), False, None), ("frame_cnt 2", dict(frame_cnt=2), False, None), ("shadows=False", dict(shadows=False), False, None), ("three lights", dict(), True, None),
            ("smooth", dict(), False, 0.5), ("ao", dict(ao=4, ao_radius=r_ao), False, None),
            ("area", dict(area=4, area_radius=r_area), False, None), ("aniso 1, bias 2", dict(), False, None))
    ctx, r = _make(F)
    for what, kw, lights, cos in todo:
        setup = multi if lights else single
        aniso, bias = (1, 2) if what.startswith("aniso") else (8, 0)
        flat_want = FR.cpu_display(F, setup, **kw)
        r.display(setup, **kw)
        ctx.synchronize()
        flat = FR.device_frame(r, setup, **kw)
        assert FR.differences(flat_want, flat) == [], what
        albedo, dbg = frame_albedo(TX, F, setup, aniso, bias)
        base = TS.smooth_frames(SM, F, setup, cos)[0] if cos is not None else F
        F2 = textured_frames(base, setup, albedo, lights, kw.get("shadows", True))
        want = FR.cpu_display(F2, setup, **kw)
        more = dict(smooth=True) if cos is not None else {}
        r.display(setup, textures=True, texture_aniso=aniso, texture_bias=bias, **more, **kw)
        ctx.synchronize()
        got = FR.device_frame(r, setup, **kw)
        assert FR.differences(want, got) == [], what
        assert_same(r.albedo.cpu().numpy(), albedo, what)
        assert FR.differences({k: v for k, v in flat.items() if k != "image"}, got) == [], what
        assert (want["image"] != flat_want["image"]).mean() > 0.05, what
        assert (dbg[:, 3] == 1).sum() > F.N // 4
    assert ctx.get_state("texture_builds") == 1  # the atlas is built once


@pytest.mark.gpu
def test_a_scene_without_uvs_keeps_its_frame(ugrt, K, torch):  # noqa: F811
    s = ugrt.scenes.cornell()
    setup = ugrt.FrameSetup(s["cameras"]["B"], s["light_camera"], s["shading_light"])
    ctx = ugrt.Context(FW, FH, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    r.display(setup)
    ctx.synchronize()
    plain = r.image.cpu().numpy().copy()
    assert not hasattr(r, "albedo") and r._tex is None and ctx.get_state("texture_builds") == 0
    for _ in range(2):
        r.display(setup, textures=True)
    ctx.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), plain)
    assert plain.any() and ctx.get_state("texture_builds") == 0 and ctx.get_state("texture_count") == 0
    # the renderer checks its host arrays at construction
    s = ugrt.scenes.textured(scale=0.1)
    R = ugrt.Renderer
    base = (ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    for kw in (dict(textures=[np.zeros((4, 4), np.uint8)]), dict(textures=[np.zeros((4, 4, 3), np.float32)]),
               dict(textures=[np.zeros((4, 4097, 3), np.uint8)]), dict(textures=s["textures"], mat_texture=[0, 1, 2]),
               dict(textures=s["textures"], mat_texture=[0, 1, 2, 3]), dict(mat_texture=[0, -1, -1, -1]),
               dict(textures=s["textures"], mat_texture=np.float32([0, 1, -1, 2])), dict(uvs=np.zeros(6, np.float32)),
               dict(uv_faces=s["uv_faces"][:-1]), dict(uv_faces=s["uv_faces"].astype(np.float32)), dict(textures=[s["textures"][0]] * 65)):
        with pytest.raises(ValueError):
            R(*base, **kw)


def test_the_filter_takes_the_aliasing_out_of_the_far_floor(ugrt, TX, K, capsys):  # noqa: F811
    """One figure, not a threshold: scenes.textured() at 128 x 128, shadows=False; the mean absolute byte error of the far half
    of the floor's pixels (material 0, t at or above their median) against the image shaded from the checker's own 8 x 8
    supersampled albedo.  The device's albedo is the checker's to the bit (test_textured_frames_equal_the_cpu_frames), so
    the images are formed on the CPU.  Asserted: level 0 alone is worse than either filtered form.  Between the two filtered
    forms no order follows from the definitions: the floor's checker has one mean everywhere, so the isotropic tap, which
    blurs along the footprint's short side too, lands on what a box over the pixel gives in the far field, while the taps
    along the long side keep what contrast is left across it and stop growing in number at texture_aniso.
    Measured (2267 pixels): level 0 alone (texture_bias=-16) 7.61, texture_aniso=1 1.30, texture_aniso=8 2.95."""
    F = tframes(K)
    setup = F.setup
    g = frame_gbuffer(F, setup)
    m = np.where(g["ids"] >= 0, g["mat_idx"][np.maximum(g["ids"], 0)], -1)
    floor = (m == 0) & (g["t"] > 0)
    far = floor & (g["t"] >= np.median(g["t"][floor]))
    assert far.sum() > 1000
    image = lambda albedo: textured_frames(F, setup, albedo, False, False).once(("shaded",), None)[0].reshape(-1, 3).astype(np.int64)
    ref = image(TX.albedo_super(g, F.scene["textures"], 8))
    err = {}
    for what, aniso, bias in (("level 0 alone", 8, -16), ("texture_aniso=1", 1, 0), ("texture_aniso=8", 8, 0)):
        got = image(frame_albedo(TX, F, setup, aniso, bias)[0])
        err[what] = float(np.abs(got - ref)[far].mean())
    with capsys.disabled():
        print("\nfar half of the floor, %d pixels, mean |byte error| against 8 x 8 supersampling: %s"
              % (int(far.sum()), ", ".join("%s %.2f" % kv for kv in err.items())))
    assert err["level 0 alone"] > max(err["texture_aniso=1"], err["texture_aniso=8"])
