"""Scene recipes shared by the golden-vector generator and the tests.

Every recipe is written against an ``api`` namespace exposing the reference's public names
(``Model, Camera, Light, Scene, Lightning, SYSTEM, SUBSYSTEM, scale, translation,
rotate_xyz``).  ``tests/golden/make_golden.py`` passes the reference's own modules (build
container only); the tests pass ``py_numpy_renderer_amd``.  Both therefore construct the
same scenes from the same files, which is what makes the captured buffers golden vectors.

Recipes follow SURVEY.md section 8(d): camera (0.5,1,2)->origin fovy 60 near 0.1 far 20, a debug
camera with identical arguments, point light (2,3,4) ambient 0.1 specular 0.1, RH/DirectX.
"""
import math
import os
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ASSETS = os.path.join(HERE, "assets")
# meshes written on first use, in a directory of the user's own: the checkout may be read-only, and a
# directory that another user created under the system temp dir could not be written
GENERATED = os.path.join(tempfile.gettempdir(), f"mi355rast_generated_{os.getuid()}")


def product_api():
    """The product's host API as a recipe namespace."""
    import py_numpy_renderer_amd as pkg
    from py_numpy_renderer_amd import transformation as tr
    return SimpleNamespace(Model=pkg.Model, Camera=pkg.Camera, Light=pkg.Light, Scene=pkg.Scene,
                           Lightning=pkg.Lightning, SYSTEM=pkg.SYSTEM, SUBSYSTEM=pkg.SUBSYSTEM, CubeMap=pkg.CubeMap,
                           PROJECTION_TYPE=pkg.PROJECTION_TYPE, scale=tr.scale, translation=tr.translation, rotate_xyz=tr.rotate_xyz)


# --------------------------------------------------------------------------- generated meshes
def _write_if_changed(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if os.path.exists(path):
        with open(path) as fh:
            if fh.read() == text:
                return path
    tmp = f"{path}.{os.getpid()}.tmp"
    with open(tmp, "w") as fh:
        fh.write(text)
    os.replace(tmp, path)
    return path


def floor_obj():
    """Two triangles (+-2, -1, +-2), normal +y (upstream's floor.obj is not shipped)."""
    text = ("v -2 -1 -2\nv 2 -1 -2\nv 2 -1 2\nv -2 -1 2\n"
            "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 1 0\n"
            "f 1/1/1 3/3/1 2/2/1\nf 1/1/1 4/4/1 3/3/1\n")
    return _write_if_changed(os.path.join(GENERATED, "floor.obj"), text)


def torus_obj(nu, nv, R=0.6, r=0.25, tilt_deg=35.0):
    """Torus with nu x nv cells (2 triangles each), tilted about x; seam duplicated in vt only."""
    path = os.path.join(GENERATED, f"torus_{nu}x{nv}.obj")
    if os.path.exists(path):
        return path
    i = np.arange(nu)[:, None]
    j = np.arange(nv)[None, :]
    u = 2 * np.pi * i / nu
    v = 2 * np.pi * j / nv
    ct, st = math.cos(math.radians(tilt_deg)), math.sin(math.radians(tilt_deg))

    def tilt(x, y, z):
        return x, ct * y - st * z, st * y + ct * z

    px, py, pz = tilt((R + r * np.cos(v)) * np.cos(u), r * np.sin(v) + 0 * u, (R + r * np.cos(v)) * np.sin(u))
    nx, ny, nz = tilt(np.cos(v) * np.cos(u), np.sin(v) + 0 * u, np.cos(v) * np.sin(u))
    lines = []
    for a, b, c in zip(px.ravel(), py.ravel(), pz.ravel()):
        lines.append("v %.6f %.6f %.6f" % (a, b, c))
    for ii in range(nu + 1):
        for jj in range(nv + 1):
            lines.append("vt %.6f %.6f" % (ii / nu, jj / nv))
    for a, b, c in zip(nx.ravel(), ny.ravel(), nz.ravel()):
        lines.append("vn %.6f %.6f %.6f" % (a, b, c))

    def vid(ii, jj):
        return (ii % nu) * nv + (jj % nv) + 1

    def tid(ii, jj):
        return ii * (nv + 1) + jj + 1

    for ii in range(nu):
        for jj in range(nv):
            a = (ii, jj); b = (ii + 1, jj); c = (ii + 1, jj + 1); d = (ii, jj + 1)
            for tri in ((a, c, b), (a, d, c)):
                lines.append("f " + " ".join("%d/%d/%d" % (vid(*p), tid(*p), vid(*p)) for p in tri))
    return _write_if_changed(path, "\n".join(lines) + "\n")


def bare_tetra_obj():
    """Tetrahedron with uv but no normals (``v/vt/``): exercises the face-normal shading path."""
    text = ("v 0 0.6 0\nv -0.5 -0.3 0.4\nv 0.5 -0.3 0.4\nv 0 -0.3 -0.5\n"
            "vt 0 0\nvt 1 0\nvt 0.5 1\n"
            "f 1/1/ 2/2/ 3/3/\nf 1/1/ 3/2/ 4/3/\nf 1/1/ 4/2/ 2/3/\nf 2/1/ 4/2/ 3/3/\n")
    return _write_if_changed(os.path.join(GENERATED, "bare_tetra.obj"), text)


def kat_files():
    """Synthetic OBJ/MTL pair for the loader known-answer test that is also
    renderable: negative (relative) indices, quads and a 5-gon (fan triangulation), three
    ``usemtl`` groups (one of them never defined in the library -> falls back to 'default'),
    a fractional ``Ns``, ``map_Kd`` + ``map_bump`` (tangent-space ``norm``) and a texture file
    that does not exist (the loader prints a hint and goes on).  The textures are copies of the
    reference's floor textures, placed next to the library as ``.mtl`` paths are relative."""
    import shutil
    os.makedirs(GENERATED, exist_ok=True)
    for src, dst in (("floor_diffuse.tga", "kat_diffuse.tga"), ("floor_nm_tangent.tga", "kat_bump.tga")):
        if not os.path.exists(os.path.join(GENERATED, dst)):
            shutil.copy(os.path.join(ASSETS, src), os.path.join(GENERATED, dst))
    mtl = ("# loader known-answer library\n\n"
           "newmtl brick\nNs 17.3\nKa 0.1 0.1 0.1\nKd 0.7 0.35 0.2\nKs 0.5 0.5 0.5\nd 1.0\nillum 2\n"
           "map_Ks kat_missing.png\n\n"
           "newmtl tiles\nNs 40\nKd 0.5 0.5 0.5\nKs 0.25 0.5 0.75\nmap_Kd kat_diffuse.tga\nmap_bump kat_bump.tga\n")
    _write_if_changed(os.path.join(GENERATED, "kat.mtl"), mtl)
    # a house: square base (quad, 'tiles'), four walls (quads, 'brick'), a pentagonal gable written with
    # negative indices, and a roof triangle pair in a group the library does not define ('slate')
    obj = ("mtllib kat.mtl\n"
           "v -0.5 -0.4 -0.5\nv 0.5 -0.4 -0.5\nv 0.5 -0.4 0.5\nv -0.5 -0.4 0.5\n"
           "v -0.5 0.3 -0.5\nv 0.5 0.3 -0.5\nv 0.5 0.3 0.5\nv -0.5 0.3 0.5\n"
           "v 0 0.75 0.5 1.0\nv 0 0.75 -0.5\n"
           "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvt 0.5 1.4 0.0\n"
           "vn 0 -1 0\nvn 0 0 -1\nvn 1 0 0\nvn 0 0 1\nvn -1 0 0\nvn 0.7071 0.7071 0\nvn -0.7071 0.7071 0\n"
           "usemtl tiles\nf 1/1/1 2/2/1 3/3/1 4/4/1\n"
           "usemtl brick\n"
           "f 1/1/2 5/4/2 6/3/2 2/2/2\nf 2/1/3 6/4/3 7/3/3 3/2/3\nf 4/2/5 8/3/5 5/4/5 1/1/5\n"
           "f -7/1/4 -8/2/4 -4/3/4 -2/5/4 -3/4/4\n"
           "usemtl slate\n"
           "f 6/1/6 10/4/6 9/3/6 7/2/6\nf -6/2/-1 -3/1/-1 -2/4/-1 -1/3/-1\n"
           "usemtl brick\nf 5/1/2 10/5/2 6/2/2\n")
    _write_if_changed(os.path.join(GENERATED, "kat.obj"), obj)
    # no uv at all: v//vn corners (-1 in the uv column), with a quad and negative indices
    nouv = ("v -0.3 -0.4 0.9\nv 0.3 -0.4 0.9\nv 0.3 0.1 0.9\nv -0.3 0.1 0.9\nv 0 0.1 1.3\n"
            "vn 0 0 -1\nvn 0 1 0\nvn 0 0 1\n"
            "f 1//1 4//1 3//1 2//1\nf -1//2 -3//2 -2//2\nf 1//3 2//3 5//3\n")
    _write_if_changed(os.path.join(GENERATED, "kat_nouv.obj"), nouv)
    # shapes the reference parses but cannot render: v/vt corners and bare v corners
    _write_if_changed(os.path.join(GENERATED, "kat_v_vt.obj"),
                      "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1 2/2 3/3 4/4\n")
    _write_if_changed(os.path.join(GENERATED, "kat_v.obj"), "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 -1\n")
    return {k: os.path.join(GENERATED, f"{k}.obj") for k in ("kat", "kat_nouv", "kat_v_vt", "kat_v")}


def gizmo_files():
    """``obj_loader_test/sphere.obj`` and ``obj_loader_test/camera.obj`` for the ``show=True`` gizmos
    (obj/core.py:532-552 loads them by these relative names; upstream does not ship them).  Returns the
    directory to run in.  Sphere: 10 x 6 lat-long mesh of radius 1; camera: a box body with a pyramid lens."""
    lines = []
    nu, nv = 10, 6
    for j in range(nv + 1):
        th = math.pi * j / nv
        for i in range(nu):
            ph = 2 * math.pi * i / nu
            lines.append("v %.6f %.6f %.6f" % (math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph)))
    for j in range(nv + 1):
        for i in range(nu + 1):
            lines.append("vt %.6f %.6f" % (i / nu, 1 - j / nv))
    for j in range(nv + 1):
        th = math.pi * j / nv
        for i in range(nu):
            ph = 2 * math.pi * i / nu
            lines.append("vn %.6f %.6f %.6f" % (math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph)))
    vid = lambda i, j: j * nu + (i % nu) + 1
    tid = lambda i, j: j * (nu + 1) + i + 1
    for j in range(nv):
        for i in range(nu):
            quad = ((i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1))
            tris = ([quad[0], quad[1], quad[2]] if j > 0 else []), ([quad[0], quad[2], quad[3]] if j < nv - 1 else [])
            if j == 0:
                tris = ([quad[0], quad[2], quad[3]],)
            elif j == nv - 1:
                tris = ([quad[0], quad[1], quad[2]],)
            for tri in tris:
                if tri:
                    lines.append("f " + " ".join("%d/%d/%d" % (vid(a, b), tid(a, b), vid(a, b)) for a, b in tri))
    _write_if_changed(os.path.join(GENERATED, "obj_loader_test", "sphere.obj"), "\n".join(lines) + "\n")
    cam = ("v -0.6 -0.4 0\nv 0.6 -0.4 0\nv 0.6 0.4 0\nv -0.6 0.4 0\n"
           "v -0.6 -0.4 1.4\nv 0.6 -0.4 1.4\nv 0.6 0.4 1.4\nv -0.6 0.4 1.4\n"
           "v 0 0 0\nv -0.5 -0.35 -0.8\nv 0.5 -0.35 -0.8\nv 0.5 0.35 -0.8\nv -0.5 0.35 -0.8\n"
           "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
           "vn 0 0 -1\nvn 0 0 1\nvn -1 0 0\nvn 1 0 0\nvn 0 -1 0\nvn 0 1 0\n"
           "f 1/1/1 4/4/1 3/3/1 2/2/1\nf 5/1/2 6/2/2 7/3/2 8/4/2\n"
           "f 1/1/3 5/2/3 8/3/3 4/4/3\nf 2/1/4 3/4/4 7/3/4 6/2/4\n"
           "f 1/1/5 2/2/5 6/3/5 5/4/5\nf 4/1/6 8/4/6 7/3/6 3/2/6\n"
           "f 9/1/5 11/3/5 10/2/5\nf 9/1/4 12/3/4 11/2/4\nf 9/1/6 13/3/6 12/2/6\nf 9/1/3 10/3/3 13/2/3\n")
    _write_if_changed(os.path.join(GENERATED, "obj_loader_test", "camera.obj"), cam)
    return GENERATED


def fins_obj():
    """A non-manifold "fin" mesh: four vertical spine edges, each shared by THREE or FOUR triangles that fan
    out from it at different angles and with mixed windings (obj/triangular.py:286-302 toggles an edge once per
    light-facing incident face: with three or four of them an edge is added, discarded and added again, and
    keeps the orientation of the LAST insert).  No closed surface anywhere: every outer edge has one face."""
    # x offset, z offset, [(fin angle in degrees, faces the light at (2, 3, 4)?)]: the winding of every fin is chosen
    # so that it does or does not face that light -- spine 1: one of three does (the edge is inserted once), spine 2:
    # three of four (inserted, discarded, inserted again), spine 3: two of four (inserted and discarded: not on the
    # silhouette), spine 4: all three (the surviving entry has the orientation of the third face)
    wanted = (
        (-0.75, 0.0, ((10, False), (130, True), (250, False))),
        (-0.25, 0.1, ((40, True), (100, True), (200, False), (320, True))),
        (0.25, -0.1, ((0, True), (90, False), (180, True), (270, False))),
        (0.75, 0.0, ((60, True), (180, True), (300, True))),
    )
    # the normal of (bottom, top, tip) is (sin a, 0, -cos a) up to scale
    spines = tuple((sx, sz, tuple((ang, 1 if ((2 * math.sin(math.radians(ang)) - 4 * math.cos(math.radians(ang))) > 0) == lit
                                   else -1) for ang, lit in fins)) for sx, sz, fins in wanted)
    verts, normals, faces = [], [], []
    for sx, sz, fins in spines:
        bottom, top = len(verts) + 1, len(verts) + 2
        verts += [(sx, -0.45, sz), (sx, 0.35, sz)]
        for ang, wind in fins:
            a = math.radians(ang)
            tip = (sx + 0.22 * math.cos(a), -0.05 + 0.002 * ang / 10.0, sz + 0.22 * math.sin(a))
            verts.append(tip)
            tri = (bottom, top, len(verts)) if wind > 0 else (top, bottom, len(verts))
            pa, pb, pc = (np.array(verts[i - 1]) for i in tri)
            n = np.cross(pb - pa, pc - pa)
            n = n / np.linalg.norm(n)
            normals.append(tuple(n))
            faces.append((tri, len(normals)))
    lines = ["v %.6f %.6f %.6f" % v for v in verts] + ["vn %.6f %.6f %.6f" % n for n in normals]
    lines += ["f " + " ".join("%d//%d" % (i, ni) for i in tri) for tri, ni in faces]
    return _write_if_changed(os.path.join(GENERATED, "fins.obj"), "\n".join(lines) + "\n")


def wall_files():
    """A 3 x 3 wall of quads, every quad in a ``usemtl`` group of its own: nine materials in one library
    (different Kd / Ks / Ns, whole and fractional exponents, two of them with a ``map_Kd``) -- with the floor's
    and the cube's that is more than the tile kernel keeps in LDS."""
    import shutil
    os.makedirs(GENERATED, exist_ok=True)
    for src, dst in (("grid.tga", "wall_grid.tga"), ("floor_diffuse.tga", "wall_floor.tga")):
        if not os.path.exists(os.path.join(GENERATED, dst)):
            shutil.copy(os.path.join(ASSETS, src), os.path.join(GENERATED, dst))
    mtl, obj = ["# nine materials"], ["mtllib wall.mtl"]
    for j in range(4):
        for i in range(4):
            obj.append("v %.6f %.6f %.6f" % (-0.9 + 0.6 * i, -0.5 + 0.45 * j, -0.3 + 0.05 * i))
    obj += ["vt 0 0", "vt 1 0", "vt 1 1", "vt 0 1", "vn 0 0 1"]
    for k in range(9):
        i, j = k % 3, k // 3
        mtl += ["", f"newmtl m{k}", "Ns %s" % (8 + 7 * k if k % 2 == 0 else 5.5 + 3.25 * k),
                "Kd %.3f %.3f %.3f" % (0.15 + 0.09 * k, 0.9 - 0.08 * k, 0.3 + 0.05 * ((k * 5) % 9)),
                "Ks %.3f %.3f %.3f" % (0.2 + 0.08 * k, 0.5, 1.0 - 0.1 * k)]
        if k == 4:
            mtl.append("map_Kd wall_grid.tga")
        if k == 7:
            mtl.append("map_Kd wall_floor.tga")
        a, b, c, d = j * 4 + i + 1, j * 4 + i + 2, (j + 1) * 4 + i + 2, (j + 1) * 4 + i + 1
        obj += [f"usemtl m{k}", f"f {a}/1/1 {b}/2/1 {c}/3/1 {d}/4/1"]
    _write_if_changed(os.path.join(GENERATED, "wall.mtl"), "\n".join(mtl) + "\n")
    return _write_if_changed(os.path.join(GENERATED, "wall.obj"), "\n".join(obj) + "\n")


def neg_uv_obj():
    """A tilted quad cut into a 3 x 3 grid whose texture coordinates run from -0.6 to 1.4 in both directions:
    negative ``vt`` truncate to negative texel indices, which Python wraps from the far side of the texture
    (obj/core.py:138-143); values above 1 are clipped (u) or go negative through ``1 - v`` (rows)."""
    lines = []
    for j in range(4):
        for i in range(4):
            lines.append("v %.6f %.6f %.6f" % (-0.8 + 1.6 * i / 3, -0.5 + 1.1 * j / 3, 0.2 - 0.25 * j / 3))
    for j in range(4):
        for i in range(4):
            lines.append("vt %.6f %.6f" % (-0.6 + 2.0 * i / 3, -0.6 + 2.0 * j / 3))
    lines.append("vn 0 0.2 1")
    for j in range(3):
        for i in range(3):
            a, b, c, d = j * 4 + i + 1, j * 4 + i + 2, (j + 1) * 4 + i + 2, (j + 1) * 4 + i + 1
            lines.append(f"f {a}/{a}/1 {b}/{b}/1 {c}/{c}/1 {d}/{d}/1")
    return _write_if_changed(os.path.join(GENERATED, "neg_uv.obj"), "\n".join(lines) + "\n")


# --------------------------------------------------------------------------- generated textures
# Non-square maps whose texels are unrelated to their neighbours: a swapped height and width, a wrong row stride or a
# wrap by the wrong dimension moves nearly every sample to a texel of another colour.  Every texel is a closed-form
# integer hash of (row, column, channel, texture id) in uint32 arithmetic: the same bytes on every host and under every
# NumPy, with no random generator whose stream could change between versions.
def hash_u32(a, b, c, d):
    """murmur3's 32-bit finaliser over four mixed-in words; arrays broadcast, arithmetic wraps at 2^32."""
    u = lambda v: np.atleast_1d(v).astype(np.uint32)            # (arrays wrap silently, scalars would warn)
    shape = np.broadcast_shapes(*(np.shape(v) for v in (a, b, c, d)))
    x = (u(a) * np.uint32(0x9E3779B1)) ^ (u(b) * np.uint32(0x85EBCA77)) ^ (u(c) * np.uint32(0xC2B2AE3D)) ^ (u(d) * np.uint32(0x27D4EB2F))
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE35)
    return (x ^ (x >> np.uint32(16))).reshape(shape)


def hash_texels(h, w, tex_id, normal_map=False):
    """uint8 (h, w, 3).  A colour map takes the top byte of the hash per channel.  A normal map is the unit vector
    (x, y, 1) / |.| with x and y from two hash bytes in [-0.75, 0.75] -- +z dominates -- encoded as
    ``rint((n + 1) / 2 * 255)``, what ``register(..., normalize=True)`` undoes."""
    row, col, ch = np.arange(h)[:, None, None], np.arange(w)[None, :, None], np.arange(3)[None, None, :]
    top = (hash_u32(row, col, ch, tex_id) >> np.uint32(24)).astype(np.int64)
    if not normal_map:
        return top.astype(np.uint8)
    n = np.empty((h, w, 3), dtype=np.float64)
    n[..., :2] = (top[..., :2] - 127.5) / 170.0
    n[..., 2] = 1.0
    n /= np.sqrt((n * n).sum(axis=-1, keepdims=True))
    return np.rint((n + 1.0) / 2.0 * 255.0).astype(np.uint8)


def hash_texture(h, w, tex_id, normal_map=False):
    """The lossless PNG of hash_texels under GENERATED, written on first use (and again if its texels differ)."""
    from PIL import Image
    path = os.path.join(GENERATED, f"hash_{'nm' if normal_map else 'rgb'}_{tex_id}_{h}x{w}.png")
    texels = hash_texels(h, w, tex_id, normal_map)
    if os.path.exists(path):
        try:
            with Image.open(path) as im:
                if np.array_equal(np.asarray(im.convert("RGB")), texels):
                    return path
        except OSError:
            pass
    os.makedirs(GENERATED, exist_ok=True)
    tmp = f"{path}.{os.getpid()}.tmp"
    Image.fromarray(texels, "RGB").save(tmp, format="PNG")
    os.replace(tmp, path)
    return path


def texture_record(path):
    """What pins a texture file: the (h, w) of the decoded image and the CRC32 of its RGB bytes."""
    import zlib
    from PIL import Image
    with Image.open(path) as im:
        texels = np.ascontiguousarray(np.asarray(im.convert("RGB")))
    return dict(shape=[int(texels.shape[0]), int(texels.shape[1])], crc32=int(zlib.crc32(texels.tobytes())))


# --------------------------------------------------------------------------- adversarial meshes
# Seeded meshes built to put counts and pixel boxes on either side of the rasteriser's limits (a pair's 24 box
# pixels, a face's 4 tiles and 64-tile work items, a tile's rounds of 64 records), with the faces a clean mesh
# never has: without area, listed twice, listed twice with opposite winding, edges with many faces.  They are
# placed through the frame of the standard camera of _std_cameras: eye (0.5, 1, 2) looking at the origin, fovy 60.
ADVERSARIAL_RESOLUTION = (136, 152)      # no multiple of 16 either way; 9 x 10 tiles: a whole-frame face needs two work items
_EYE = np.array([0.5, 1.0, 2.0])
_FWD = -_EYE / np.linalg.norm(_EYE)
_RIGHT = np.cross(_FWD, [0.0, 1.0, 0.0]) / np.linalg.norm(np.cross(_FWD, [0.0, 1.0, 0.0]))
_UP = np.cross(_RIGHT, _FWD)
_PX = 2 * math.tan(math.radians(30)) / ADVERSARIAL_RESOLUTION[0]      # world units per pixel and unit of distance


_PIVOT = -_EYE / 32                      # on the camera's axis, exact in float32 and in six decimals: see _dense_tile


def _at(px, py, d):
    """World point that the standard camera sees at pixel (px, py) of the 136 x 152 frame (x to the right, y upwards
    like the reference's buffer rows), *d* world units in front of the camera plane."""
    h, w = ADVERSARIAL_RESOLUTION
    return _EYE + d * (_FWD + (px - w / 2) * _PX * _RIGHT + (py - h / 2) * _PX * _UP)


class _ObjWriter:
    """``v/vt/`` faces like bare_tetra_obj: uv, no normals.  Corners are (vertex, uv) pairs of 1-based indices."""

    def __init__(self, rng):
        self.rng, self.v, self.vt, self.f = rng, [], [], []
        self.group, self.groups = "", []                 # the label of every face written, in file order

    def vertex(self, p):
        self.v.append("v %.6f %.6f %.6f" % tuple(p))
        return len(self.v)

    def uv(self):
        """A texture coordinate outside [0, 1] on either side: u from -0.95 to 2.5, v from -1.5 to 1.95.  Below 0 a
        texel index wraps from the far side, above 1 it clips (obj/core.py:138-143); u below -1 or v above 2 would
        index past the far side, and upstream raises IndexError there."""
        self.vt.append("vt %.6f %.6f" % (self.rng.uniform(-0.95, 2.5), self.rng.uniform(-1.5, 1.95)))
        return len(self.vt)

    def face(self, vi, ti=None):
        ti = ti if ti is not None else [self.uv() for _ in vi]
        self.f.append("f " + " ".join("%d/%d/" % c for c in zip(vi, ti)))
        self.groups.append(self.group)
        return list(vi), list(ti)

    def triangle(self, a, b, c):
        """An isolated triangle: three vertices and three uv of its own."""
        return self.face([self.vertex(a), self.vertex(b), self.vertex(c)])

    def text(self):
        return "\n".join(self.v + self.vt + self.f) + "\n"


def _backdrop(obj, d):
    """One face over the whole frame, *d* in front of the camera, listed with both windings on vertices of its own:
    its pixel box is the frame (90 tiles, two 64-tile work items), its corners lie outside the frustum."""
    a, b, c = _at(-190, -40, d), _at(342, -40, d), _at(76, 330, d)
    obj.triangle(a, b, c)
    obj.triangle(a, c, b)


def _soup_triangles(obj, rng, n):
    """*n* isolated triangles of four sizes from half a world unit down to sub-pixel, three quarters of them facing
    the camera, then the kinds without area and the repeats."""
    made = []
    for i in range(n):
        size = (0.5, 0.12, 0.03, 0.004)[i % 4]
        d = rng.uniform(1.5, 4.0)
        centre = _at(rng.uniform(5, 147), rng.uniform(5, 131), d)
        ang = np.sort(rng.uniform(0, 2 * np.pi, 3))
        if i % 4 == 3 and rng.random() < 0.5:
            ang = ang[::-1]
        pts = [centre + size * rng.uniform(0.3, 1.0) * (math.cos(t) * _RIGHT + math.sin(t) * _UP)
               + size * rng.uniform(-0.3, 0.3) * _FWD for t in ang]
        obj.triangle(*pts)
        made.append(pts)
    for k in range(3):                                   # two equal corners, in every position
        a, b = made[k][0], made[k][1] + 0.05 * _UP
        obj.triangle(*[(a, a, b), (a, b, a), (b, a, a)][k])
    for k in range(3):                                   # collinear corners; a near-collinear sliver
        a, b = made[3 + k][0], made[3 + k][1]
        obj.triangle(a, a + 0.5 * (b - a), b)
        obj.triangle(a, a + 0.5 * (b - a) + 2e-4 * _UP, b)
    for k in range(0, n, 5):                             # exact repeats of an earlier face, some with the winding turned
        a, b, c = made[k]
        obj.triangle(*((a, b, c) if k % 10 else (a, c, b)))
    return made


def soup_obj(seed, behind=False):
    """Triangle soup: isolated triangles from sub-pixel to half the frame, faces with two equal corners, collinear
    corners, a sliver, exact repeats with the same and the opposite winding, and one face over the whole frame.
    Every vertex lies in front of the camera plane -- unless *behind*: then three large faces with one or two corners
    behind it (clip-space w < 0) come FIRST in the file, so that no earlier face has coloured the pixels they own."""
    rng = np.random.default_rng(20261018 + seed)
    obj = _ObjWriter(rng)
    if behind:
        for k, (px, py, back) in enumerate(((20, 30, 1), (125, 95, 1), (80, 125, 2))):
            # three world units across, straddling the camera plane: corners at d = 2.5 and at d = -0.5
            a = _at(px, py, 2.5)
            b = _at(px + 40, py + 10, 2.5) if back == 1 else _EYE - 0.5 * _FWD + 0.4 * _RIGHT + 0.2 * k * _UP
            c = _EYE - 0.5 * _FWD - 0.3 * _RIGHT - 0.5 * _UP + 0.3 * k * _RIGHT
            obj.triangle(a, b, c)
    _soup_triangles(obj, rng, 48)
    _backdrop(obj, 6.0)
    name = f"soup_{'behind_' if behind else ''}{seed}.obj"
    return _write_if_changed(os.path.join(GENERATED, name), obj.text())


def welded_obj(seed):
    """70 faces drawn from a pool of 14 vertices and 9 uv: many edges with three and more faces (the edge stage's
    extra-incidence lists), one edge with seven, an index used twice in a face, faces repeated with the same and
    with the opposite winding."""
    rng = np.random.default_rng(20261019 + seed)
    obj = _ObjWriter(rng)
    pool = [obj.vertex(rng.uniform(-0.65, 0.65, 3) * (1.0, 0.8, 1.0)) for _ in range(14)]
    uvs = [obj.uv() for _ in range(9)]
    faces = []

    def add(vi):
        faces.append(obj.face(list(vi), [uvs[int(t)] for t in rng.integers(0, 9, 3)]))

    for k in range(2, 9):                                # seven faces on the edge (pool[0], pool[1]), windings mixed
        add((pool[0], pool[1], pool[k]) if k % 3 else (pool[1], pool[0], pool[k]))
    while len(faces) < 58:
        add(rng.choice(pool, 3, replace=False))
    for k in range(4):                                   # an index used twice in a face
        a, b = rng.choice(pool, 2, replace=False)
        add([(a, a, b), (a, b, a), (b, a, a), (a, b, b)][k])
    for k in range(8):                                   # repeats: the same corners again, every other one turned
        vi, ti = faces[3 + 5 * k]
        obj.face(vi if k % 2 else [vi[0], vi[2], vi[1]], ti if k % 2 else [ti[0], ti[2], ti[1]])
    return _write_if_changed(os.path.join(GENERATED, f"welded_{seed}.obj"), obj.text())


def _dense_tile(seed):
    """The writer behind dense_tile_obj, with every face labelled (``groups``)."""
    rng = np.random.default_rng(20261020 + seed)
    obj = _ObjWriter(rng)

    def tiny(cx, cy, spread, lo, hi, count, d_lo=2.38, d_hi=2.5):        # on both sides of the stack's plane
        for i in range(count):
            d = rng.uniform(d_lo, d_hi)
            px, py = cx + rng.uniform(-spread, spread), cy + rng.uniform(-spread, spread)
            r = rng.uniform(lo, hi) / 2
            ang = np.sort(rng.uniform(0, 2 * np.pi, 3))
            if i % 4 == 3:
                ang = ang[::-1]                          # a quarter face away from the camera
            obj.triangle(*[_at(px + r * math.cos(t), py + r * math.sin(t), d) for t in ang])

    # (a face whose box holds no sample of it never reaches a tile: of these about half do)
    obj.group = "tiny"
    tiny(76, 68, 2.5, 1.5, 4, 520)                       # more than 128 small pairs in the centre tile
    tiny(108, 68, 2.5, 1.5, 3.5, 240)                    # 65 to 128 in the tile two to the right
    tiny(76, 68, 24, 1, 8, 200)                          # small and big pairs side by side in the tiles around
    obj.group = "tile_sized"
    for i in range(12):
        px, py = rng.uniform(20, 132), rng.uniform(20, 116)
        obj.triangle(_at(px, py, 2.6), _at(px + 16, py + rng.uniform(-3, 3), 2.6), _at(px + rng.uniform(0, 16), py + 16, 2.6))
    # the stack: nine faces on 12 coplanar points around the centre tile, in the plane 2.44 in front of the camera, each
    # listed eight times, copy k of every face before copy k + 1 of any: 72 big pairs in that tile, and at every
    # pixel the nearest face ties with its seven copies -- the last of them wins, in whatever order the tile's list was filled
    obj.group = "stack"
    pix = np.array([(76 + 14 * math.cos(t) + rng.uniform(-2, 2), 68 + 14 * math.sin(t) + rng.uniform(-2, 2))
                    for t in np.linspace(0, 2 * np.pi, 12, endpoint=False)])
    pts = [_at(px, py, 2.44) for px, py in pix]
    ids = [obj.vertex(p) for p in pts]
    uvs = [obj.uv() for _ in ids]
    stack = [tuple(int(t) for t in np.sort(rng.choice(12, 3, replace=False))) for _ in range(9)]     # ascending: towards the camera
    for _ in range(8):
        for tri in stack:
            obj.face([ids[t] for t in tri], [uvs[t] for t in tri])
    # tiny faces in the stack's plane: convex combinations of a stack face's corners, shrunk until the pixel box is at
    # most 4 x 4, and copies of one of them.  Their z is the stack's to about 1e-7 and never to the bit (the corners' z
    # differ after rounding to six decimals, and so do the roundings of two faces' barycentrics): the copies tie with each
    # other, small pair against small pair, and none of them with the stack.
    obj.group = "in_plane"
    copies = None
    for k in range(24):
        tri = list(stack[k % 9])
        extent = float((pix[tri].max(axis=0) - pix[tri].min(axis=0)).max())
        share = min(0.5, 3.9 / extent)
        w = (1 - share) * rng.dirichlet((1, 1, 1)) + share * np.eye(3)
        sub = [w[j, 0] * pts[tri[0]] + w[j, 1] * pts[tri[1]] + w[j, 2] * pts[tri[2]] for j in range(3)]
        obj.triangle(*sub)
        copies = sub if copies is None else copies
    for _ in range(3):
        obj.triangle(*copies)
    # the pivot: where a small and a big pair do tie to the bit.  _PIVOT lies on the camera's axis and has coordinates
    # that are powers of two, so it lands on the sample of pixel (76, 68), the frame's centre, exactly: its clip-space x
    # and y vanish, and its w is one of the doubles for which w * (1 / w) rounds to 1 (the origin's is not).  A face whose
    # FIRST corner it is has the barycentrics (1, 0, 0) there, and its z at that pixel is the corner's own, whatever
    # the other two corners are.  Six faces with a box of at most 4 x 4 pixels and four that reach 9 to 11.5 pixels
    # into the tile, in seeded order, in front of everything else at that pixel: ten pairs of both classes tie there,
    # and the last in the file wins.  (A pixel box is half open: the sample is in it because the other corners lie to
    # its right and above.  The vertex lies beyond the origin, where the orthographic camera's near plane is.  No tie
    # under the f64 variant: its rotation takes the vertex off the axis.)
    obj.group = "pivot"
    d = float(np.dot(_PIVOT - _EYE, _FWD))
    for big in rng.permutation([False] * 6 + [True] * 4):
        if big:
            r, t1, t2 = rng.uniform(9, 11.5, 2), rng.uniform(20, 50), rng.uniform(100, 150)
        else:
            r, t1, t2 = rng.uniform(2, 3.8, 2), rng.uniform(-15, 30), rng.uniform(60, 105)
        t1, t2 = math.radians(t1), math.radians(t2)
        da, db = d + rng.uniform(0.004, 0.008, 2)
        obj.triangle(_PIVOT, _at(76 + r[0] * math.cos(t1), 68 + r[0] * math.sin(t1), da), _at(76 + r[1] * math.cos(t2), 68 + r[1] * math.sin(t2), db))
    # the fan: 80 faces on the edge (p, q), every one wound to face the light at (2, 3, 4), so that each throws two quads
    obj.group = "fan"
    p, q = _at(20, 118, 2.0), _at(52, 100, 2.2)
    ip, iq, tp, tq = obj.vertex(p), obj.vertex(q), obj.uv(), obj.uv()
    axis = (q - p) / np.linalg.norm(q - p)
    side = np.cross(axis, _FWD) / np.linalg.norm(np.cross(axis, _FWD))
    light = np.array([2.0, 3.0, 4.0])
    for k in range(80):
        t = 2 * np.pi * k / 80
        tip = 0.5 * (p + q) + 0.25 * (math.cos(t) * side + math.sin(t) * np.cross(axis, side)) + 0.002 * k * axis
        it, tt = obj.vertex(tip), obj.uv()
        lit = np.dot(np.cross(q - p, tip - p), light) > 0
        obj.face([ip, iq, it] if lit else [iq, ip, it], [tp, tq, tt] if lit else [tq, tp, tt])
    obj.group = "backdrop"
    _backdrop(obj, 5.0)
    return obj


def dense_tile_obj(seed):
    """Hundreds of triangles of 1 to 8 pixels inside a few tiles, a dozen tile-sized ones, a stack of 72 coplanar,
    partly overlapping faces (nine, each listed eight times) over the tile at the frame's centre with tiny faces in its
    plane, ten faces of both pair classes that tie to the bit at the frame's centre, a fan of 80 faces on one long edge
    whose shadow quads run through the same tiles, and a face over the whole frame behind them all.  Pixel (76, 68), the
    frame's centre, lies 4 pixels or more inside its tile in both directions: a cluster within 3 pixels of it falls into
    one tile."""
    return _write_if_changed(os.path.join(GENERATED, f"dense_tile_{seed}.obj"), _dense_tile(seed).text())


def dense_tile_groups(seed):
    """The label of every face of dense_tile_obj(seed), in file order: tiny, tile_sized, stack, in_plane, pivot, fan,
    backdrop."""
    return np.array(_dense_tile(seed).groups)


# --------------------------------------------------------------------------- building blocks
def _std_cameras(api, **over):
    kw = dict(fovy=60, near=0.1, far=20, backface_culling=True)
    kw.update(over)
    return (api.Camera((0.5, 1, 2), (0, 0, 0), **kw), api.Camera((0.5, 1, 2), (0, 0, 0), **kw))


def _std_light(api, **over):
    kw = dict(ambient_strength=0.1, specular_strength=0.1)
    kw.update(over)
    return api.Light((2, 3, 4), **kw)


def _diablo(api):
    d = os.path.join(ASSETS, "diablo3_pose")
    m = api.Model.load_model(os.path.join(d, "diablo3_pose.obj"))
    m.textures.register("normals", os.path.join(d, "diablo3_pose_nm_tangent.tga"), tangent=True)
    m.textures.register("diffuse", os.path.join(d, "diablo3_pose_diffuse.tga"), normalize=False)
    return m


def _floor(api, textured=True):
    m = api.Model.load_model(floor_obj())
    if textured:
        m.textures.register("diffuse", os.path.join(ASSETS, "floor_diffuse.tga"), normalize=False)
    return m


def _torus(api, nu, nv):
    m = api.Model.load_model(torus_obj(nu, nv))
    m.textures.register("diffuse", os.path.join(ASSETS, "grid.tga"), normalize=False)
    m.textures.register("normals", os.path.join(ASSETS, "floor_nm_tangent.tga"), tangent=True)
    return m


def _scene(api, cam, dbg, light, resolution, models, **kw):
    sc = api.Scene(cam, light, debug_camera=dbg, resolution=resolution, **kw)
    for m in models:
        sc.add_model(m)
    # The captures under tests/golden/ were taken with the reference's debug-frustum overlay patched out
    # (make_golden.py), the *_overlay ones with it left on; the product's switch for it defaults to ON like
    # upstream, so the recipes turn it off and the overlay tests turn it back on.  (On the reference's
    # Scene this is just an unused attribute.)
    sc.draw_debug_frustum = False
    return sc


# --------------------------------------------------------------------------- recipes
def cube_small(api, resolution=(120, 160)):
    """G1: cube.obj with .mtl (map_Kd, map_Ks, Ns 32), point light."""
    cam, dbg = _std_cameras(api)
    cube = api.Model.load_model(os.path.join(ASSETS, "cube", "cube.obj"))
    return _scene(api, cam, dbg, _std_light(api), resolution, [cube])


def cube_outward(api, resolution=(120, 160)):
    """Cube with normals flipped outward (lit faces show the specular map) and f64 vertices
    (``Model @ scale`` promotes float32 vertices to float64)."""
    cam, dbg = _std_cameras(api)
    cube = api.Model.load_model(os.path.join(ASSETS, "cube", "cube.obj"))
    cube.normals = -cube.normals
    cube = cube @ api.scale(0.45)
    floor = _floor(api, textured=False)
    return _scene(api, cam, dbg, _std_light(api), resolution, [cube, floor])


def diablo_small(api, resolution=(240, 320)):
    """G2: diablo, tangent-space normal map, shadows onto itself."""
    cam, dbg = _std_cameras(api)
    return _scene(api, cam, dbg, _std_light(api), resolution, [_diablo(api)])


def diablo_floor_lh_gl(api, resolution=(270, 480)):
    """G3: upstream main.py's parameters (obj/main.py:63-92,117-129): LH/OpenGL, directional light
    (w=2 extrusion), culling off, and a debug camera that really clips."""
    light = api.Light((5, 5, 0), light_type=api.Lightning.DIRECTIONAL_LIGHTNING, center=(0, 0.5, 0.5),
                      fovy=90, linear=0.000000001, quadratic=0.0000000001,
                      ambient_strength=0.1, specular_strength=0.1)
    cam = api.Camera((0.5, 3, 5), up=np.array((0, 1, 0)), fovy=90, near=0.0001, far=400,
                     backface_culling=False, center=(0, 0, 0))
    dbg = api.Camera((0, 3, 0.01), up=np.array((0, 1, 0)), fovy=80, near=1, far=3,
                     backface_culling=True, center=(0, 0, 0))
    return _scene(api, cam, dbg, light, resolution, [_diablo(api), _floor(api)],
                  system=api.SYSTEM.LH, subsystem=api.SUBSYSTEM.OPENGL)


def diablo_floor(api, resolution=(270, 480)):
    """c3 at reduced size: diablo + floor, RH/DirectX, point light, shadows."""
    cam, dbg = _std_cameras(api)
    return _scene(api, cam, dbg, _std_light(api), resolution, [_diablo(api), _floor(api)])


def torus_spot(api, resolution=(180, 320), nu=40, nv=25):
    """G4: 2 000-triangle torus + floor under a spot light."""
    cam, dbg = _std_cameras(api)
    light = api.Light((2, 3, 4), light_type=api.Lightning.SPOT_LIGHTNING,
                      ambient_strength=0.1, specular_strength=0.1)
    return _scene(api, cam, dbg, light, resolution, [_torus(api, nu, nv), _floor(api)])


def torus_floor(api, resolution=(1080, 1920), nu=500, nv=200):
    """c4 (nu=500, nv=200 -> 200 000 triangles) and its reduced variants."""
    cam, dbg = _std_cameras(api)
    return _scene(api, cam, dbg, _std_light(api), resolution, [_torus(api, nu, nv), _floor(api)])


def _cubemap(api):
    d = os.path.join(ASSETS, "cubemap")            # face assignment of obj/main.py:101-106
    return api.CubeMap(back=os.path.join(d, "neg-z.jpg"), front=os.path.join(d, "pos-z.jpg"),
                       top=os.path.join(d, "pos-y.jpg"), bottom=os.path.join(d, "neg-y.jpg"),
                       left=os.path.join(d, "neg-x.jpg"), right=os.path.join(d, "pos-x.jpg"))


def cube_skybox(api, resolution=(135, 240)):
    """G5: the outward cube + floor in front of the 512^2 cubemap skybox."""
    sc = cube_outward(api, resolution=resolution)
    sc.skybox = _cubemap(api)
    return sc


def torus_skybox(api, resolution=(2160, 3840), nu=1000, nv=500):
    """c5: 1M-triangle torus + floor + cubemap skybox at 3840x2160 (and reduced variants)."""
    sc = torus_floor(api, resolution=resolution, nu=nu, nv=nv)
    sc.skybox = _cubemap(api)
    return sc


def tetra_bare(api, resolution=(120, 160)):
    """Model without vertex normals and without textures on a textured floor: Kd colour,
    face-normal shading, GL/RH projection."""
    cam, dbg = _std_cameras(api)
    tet = api.Model.load_model(bare_tetra_obj())
    return _scene(api, cam, dbg, _std_light(api), resolution, [tet, _floor(api)],
                  system=api.SYSTEM.RH, subsystem=api.SUBSYSTEM.OPENGL)


def diablo_closeup(api, resolution=(200, 200)):
    """Camera close enough that triangles cross the frustum sides: exercises the per-fragment
    clip (obj/triangular.py:80-87) and screen-edge bounding boxes."""
    kw = dict(fovy=40, near=0.3, far=5, backface_culling=True)
    cam = api.Camera((0.2, 0.5, 0.9), (0, 0.3, 0), **kw)
    dbg = api.Camera((0.2, 0.5, 0.9), (0, 0.3, 0), **kw)
    return _scene(api, cam, dbg, _std_light(api), resolution, [_diablo(api)])


def diablo_nm_object(api, resolution=(240, 320)):
    """Object-space normal map (``register('normals', ..., tangent=False)``, obj/core.py:175-181):
    the texel is the normal, no TBN."""
    cam, dbg = _std_cameras(api)
    d = os.path.join(ASSETS, "diablo3_pose")
    m = api.Model.load_model(os.path.join(d, "diablo3_pose.obj"))
    m.textures.register("normals", os.path.join(d, "diablo3_pose_nm.tga"), tangent=False)
    m.textures.register("diffuse", os.path.join(d, "diablo3_pose_diffuse.tga"), normalize=False)
    return _scene(api, cam, dbg, _std_light(api), resolution, [m])


def diablo_closeup_noclip(api, resolution=(200, 200)):
    """``Model.clip = False`` (obj/triangular.py:80): the per-fragment frustum test is skipped, so
    the fragments the close-up camera's planes would cut are kept."""
    sc = diablo_closeup(api, resolution=resolution)
    sc.models[0].clip = False
    return sc


def kat_house(api, resolution=(150, 200)):
    """The loader known-answer meshes rendered: several material groups, fractional Ns
    (``**`` takes the pow() path), map_bump from the library, a model without uv."""
    files = kat_files()
    cam, dbg = _std_cameras(api)
    house = api.Model.load_model(files["kat"])
    porch = api.Model.load_model(files["kat_nouv"])
    return _scene(api, cam, dbg, _std_light(api, specular_strength=0.4), resolution, [house, porch, _floor(api)])


def cube_tetra_nodepth(api, resolution=(120, 160)):
    """``Model.depth_test = False`` (obj/core.py:235-241, obj/triangular.py:117): a tetrahedron that is tested
    against the z-buffer but never writes to it, between two z-writing models in model order, poking
    through the cube (so it wins some pixels, loses others, and later faces draw over it)."""
    cam, dbg = _std_cameras(api)
    cube = api.Model.load_model(os.path.join(ASSETS, "cube", "cube.obj"))
    cube.normals = -cube.normals
    cube = cube @ api.scale(0.45)
    tet = api.Model.load_model(bare_tetra_obj())
    tet.depth_test = False
    tet = tet @ api.scale(1.3)
    return _scene(api, cam, dbg, _std_light(api), resolution, [cube, tet, _floor(api)])


def gizmos_small(api, resolution=(150, 200)):
    """``show=True`` on the light and on the debug camera (obj/core.py:532-552): a sphere at the light's
    place and a camera body at the debug camera's, both ``clip = False``, in front of the cube and the floor.
    The scene is constructed from the directory that holds ``obj_loader_test/`` (upstream's relative paths)."""
    here = os.getcwd()
    os.chdir(gizmo_files())
    try:
        kw = dict(fovy=60, near=0.1, far=20, backface_culling=True)
        cam = api.Camera((0.5, 1, 2), (0, 0, 0), **kw)
        dbg = api.Camera((1.1, 0.5, 0.2), (0, 0, 0), show=True, **kw)
        light = api.Light((-0.9, 1.0, 0.6), ambient_strength=0.1, specular_strength=0.1, show=True)
        sc = api.Scene(cam, light, debug_camera=dbg, resolution=resolution)
    finally:
        os.chdir(here)
    cube = api.Model.load_model(os.path.join(ASSETS, "cube", "cube.obj")) @ api.scale(0.5)
    for m in (cube, _floor(api)):
        sc.add_model(m)
    sc.draw_debug_frustum = False
    return sc


def tetra_ortho(api, resolution=(120, 160)):
    """Orthographic camera (obj/transformation.py:139-154; only OpenGL + LH exists upstream):
    near = |position| (obj/core.py:389), float32 projection matrix."""
    kw = dict(projection_type=api.PROJECTION_TYPE.ORTHOGRAPHIC, fovy=35, far=20, backface_culling=True)
    cam = api.Camera((0.5, 1, 2), (0, 0, 0), **kw)
    dbg = api.Camera((0.5, 1, 2), (0, 0, 0), **kw)
    tet = api.Model.load_model(bare_tetra_obj())
    return _scene(api, cam, dbg, _std_light(api), resolution, [tet, _floor(api)],
                  system=api.SYSTEM.LH, subsystem=api.SUBSYSTEM.OPENGL)


def fins_nonmanifold(api, resolution=(150, 200)):
    """Silhouette edges with three and four incident faces (obj/triangular.py:286-302), culling off so that
    both sides of the fins are drawn, over a floor that catches their shadow volumes."""
    cam, dbg = _std_cameras(api, backface_culling=False)
    fins = api.Model.load_model(fins_obj())
    return _scene(api, cam, dbg, _std_light(api), resolution, [fins, _floor(api)])


def wall_nine_materials(api, resolution=(150, 200)):
    """More materials in one scene than the tile kernel stages in LDS: nine in the wall's library, the cube's
    (map_Kd + map_Ks) and the floor's."""
    cam, dbg = _std_cameras(api)
    wall = api.Model.load_model(wall_files())
    cube = api.Model.load_model(os.path.join(ASSETS, "cube", "cube.obj"))
    cube.normals = -cube.normals
    cube = cube @ api.scale(0.3) @ api.translation((0.2, -0.3, 0.6))
    return _scene(api, cam, dbg, _std_light(api, specular_strength=0.3), resolution, [wall, cube, _floor(api)])


def quad_negative_uv(api, resolution=(150, 200)):
    """Texture coordinates below 0 and above 1 on a textured, normal-mapped quad (obj/core.py:138-143)."""
    cam, dbg = _std_cameras(api)
    quad = api.Model.load_model(neg_uv_obj())
    quad.textures.register("diffuse", os.path.join(ASSETS, "grid.tga"), normalize=False)
    quad.textures.register("normals", os.path.join(ASSETS, "floor_nm_tangent.tga"), tangent=True)
    return _scene(api, cam, dbg, _std_light(api), resolution, [quad, _floor(api)])


# --------------------------------------------------------------------------- shading inputs
# Recipes for what the captures above hold constant: texture shapes (every file under assets/ is square), the light's
# colour, attenuation and ambient strength, a colour sky and the cameras' viewport offsets.
TEXTURED = {}                  # recipe name -> {label: texture file}, filled in when the recipe is built


def _register_hash_maps(model, recipe, prefix, diffuse=None, normals=None, specular=None, tangent=True):
    """Hash textures of the given (h, w, texture id) on a model; the files are noted under TEXTURED[recipe]."""
    files = TEXTURED.setdefault(recipe, {})
    if diffuse is not None:
        files[f"{prefix}_diffuse"] = hash_texture(*diffuse)
        model.textures.register("diffuse", files[f"{prefix}_diffuse"], normalize=False)
    if normals is not None:
        files[f"{prefix}_normals"] = hash_texture(*normals, normal_map=True)
        model.textures.register("normals", files[f"{prefix}_normals"], tangent=tangent)
    if specular is not None:
        files[f"{prefix}_specular"] = hash_texture(*specular)
        model.textures.register("specular", files[f"{prefix}_specular"], normalize=False)
    return model


def torus_rect_maps(api, resolution=(150, 200), name="torus_rect_maps"):
    """Three maps of different non-square shapes on one material -- diffuse 40 x 96 (h x w), tangent-space normal map
    96 x 40, specular map 33 x 57 -- and a 64 x 31 floor, under a coloured point light close to the torus whose
    ``constant`` is below 1: the attenuation exceeds 1 on the near side and some channels end at the upper clip."""
    cam, dbg = _std_cameras(api)
    light = api.Light((0.9, 1.5, 1.3), color=(1.0, 0.7, 0.4), ambient_strength=0.25, specular_strength=0.6,
                      constant=0.6, linear=0.3, quadratic=0.02)
    torus = _register_hash_maps(api.Model.load_model(torus_obj(40, 25)), name, "torus",
                                diffuse=(40, 96, 1), normals=(96, 40, 2), specular=(33, 57, 3))
    floor = _register_hash_maps(api.Model.load_model(floor_obj()), name, "floor", diffuse=(64, 31, 4))
    return _scene(api, cam, dbg, light, resolution, [torus, floor])


def quad_rect_object_nm(api, resolution=(150, 200), name="quad_rect_object_nm"):
    """neg_uv_obj's quad (uv from -0.6 to 1.4: rows and columns wrap from the far side) with a 24 x 80 diffuse map, an
    80 x 24 OBJECT-space normal map and a specular map one texel wide (5 x 1: ``w - 1 == 0``, every column index is 0),
    LH/OpenGL, culling off, under a coloured directional light with an attenuation of its own."""
    cam, dbg = _std_cameras(api, backface_culling=False)
    light = api.Light((-0.5, 1.0, 1.5), light_type=api.Lightning.DIRECTIONAL_LIGHTNING, center=(0, 0, 0),
                      color=(0.5, 0.9, 1.0), ambient_strength=0.3, specular_strength=0.4,
                      constant=1.2, linear=0.05, quadratic=0.25)
    quad = _register_hash_maps(api.Model.load_model(neg_uv_obj()), name, "quad",
                               diffuse=(24, 80, 5), normals=(80, 24, 6), specular=(5, 1, 7), tangent=False)
    floor = _register_hash_maps(api.Model.load_model(floor_obj()), name, "floor", diffuse=(64, 31, 4))
    return _scene(api, cam, dbg, light, resolution, [quad, floor], system=api.SYSTEM.LH, subsystem=api.SUBSYSTEM.OPENGL)


def _shift(scene, x_offset, y_offset):
    for cam in (scene.camera, scene.debug_camera):
        cam.x_offset, cam.y_offset = x_offset, y_offset
    return scene


def cube_skybox_offset(api, resolution=(135, 240), offsets=(13, 52)):
    """cube_skybox with both cameras' viewport shifted: the scene and the cubemap's two screen triangles move."""
    return _shift(cube_skybox(api, resolution=resolution), *offsets)


def torus_spot_offset_sky(api, resolution=(180, 320), offsets=(-45, -9), sky=(0.9, 0.3, 0.1), nu=40, nv=25):
    """torus_spot shifted so that part of the scene leaves the frame on two sides, under a coloured spot light, in
    front of a colour sky (``Scene(skymap=<colour>)``, obj/core.py:597-598)."""
    cam, dbg = _std_cameras(api)
    light = api.Light((2, 3, 4), light_type=api.Lightning.SPOT_LIGHTNING, color=(0.9, 1.0, 0.5),
                      ambient_strength=0.1, specular_strength=0.1)
    sc = _scene(api, cam, dbg, light, resolution, [_torus(api, nu, nv), _floor(api)], skymap=sky)
    return _shift(sc, *offsets)


def _unit(seed, k):
    """The k-th draw of a sweep seed: a float in [0, 1) from the integer hash (no random generator)."""
    return float(hash_u32(seed, k, 0x5EED, 0xD1CE)) / 2.0 ** 32


def shading_sweep_parameters(seed, resolution=ADVERSARIAL_RESOLUTION):
    """What seed *seed* of the shading-input sweep draws: four map shapes with 2 to 97 rows and 1 to 97 columns (seeds 1,
    2, 3 and 5 mod 8 force a 2 x N, an N x 1 and two 2 x 1 maps), a light kind, colour and attenuation, viewport offsets
    within half the frame either way, and a sky colour in [0, 1] (one component of seed 4 mod 8 is exactly 0, one of seed
    6 exactly 1).  No map is one texel HIGH: upstream's ``Material.__setattr__`` (obj/materials.py:57-60) takes an array
    whose first axis has length 1 for a one-entry ``.mtl`` value and raises on it, and so does this package's."""
    draws = iter(range(64))
    u = lambda: _unit(seed, next(draws))
    shapes = {key: (2 + int(u() * 96), 1 + int(u() * 97)) for key in ("torus_diffuse", "torus_normals", "torus_specular", "floor_diffuse")}
    forced = {1: ("torus_diffuse", (2, None)), 2: ("torus_normals", (None, 1)), 3: ("torus_specular", (2, 1)),
              5: ("floor_diffuse", (2, 1))}.get(seed % 8)
    if forced:
        key, (fh, fw) = forced
        shapes[key] = (fh or shapes[key][0], fw or shapes[key][1])
    h, w = resolution
    sky = [round(u(), 3) for _ in range(3)]
    if seed % 8 == 4:
        sky[seed // 8 % 3] = 0.0
    if seed % 8 == 6:
        sky[seed // 8 % 3] = 1.0
    return dict(shapes=shapes, kind=seed % 3, position=(4 * u() - 2, 1.5 + 2.5 * u(), 4 * u() - 2),
                color=tuple(round(0.2 + 0.8 * u(), 3) for _ in range(3)),
                ambient_strength=round(0.4 * u(), 3), specular_strength=round(0.7 * u(), 3),
                constant=round(0.5 + u(), 3), linear=round(0.4 * u(), 3), quadratic=round(0.4 * u(), 3),
                offsets=(int((2 * u() - 1) * (w // 2)), int((2 * u() - 1) * (h // 2))), sky=tuple(sky),
                tangent=bool(seed % 2 == 0), lh_gl=bool(seed % 4 == 3))


def shading_sweep(api, seed, resolution=ADVERSARIAL_RESOLUTION):
    """One seed of the sweep: a 24 x 16 torus with three hash maps and the floor with one, under what
    shading_sweep_parameters draws.  An object-space normal map on odd seeds, LH/OpenGL on every fourth."""
    p = shading_sweep_parameters(seed, resolution)
    name = f"shading_sweep_{seed}"
    kinds = (api.Lightning.POINT_LIGHTNING, api.Lightning.SPOT_LIGHTNING, api.Lightning.DIRECTIONAL_LIGHTNING)
    cam, dbg = _std_cameras(api)
    light = api.Light(p["position"], light_type=kinds[p["kind"]], center=(0, 0, 0), color=p["color"],
                      ambient_strength=p["ambient_strength"], specular_strength=p["specular_strength"],
                      constant=p["constant"], linear=p["linear"], quadratic=p["quadratic"])
    s = p["shapes"]
    torus = _register_hash_maps(api.Model.load_model(torus_obj(24, 16)), name, "torus",
                                diffuse=(*s["torus_diffuse"], 100 + seed), normals=(*s["torus_normals"], 200 + seed),
                                specular=(*s["torus_specular"], 300 + seed), tangent=p["tangent"])
    floor = _register_hash_maps(api.Model.load_model(floor_obj()), name, "floor", diffuse=(*s["floor_diffuse"], 400 + seed))
    system = dict(system=api.SYSTEM.LH, subsystem=api.SUBSYSTEM.OPENGL) if p["lh_gl"] else {}
    sc = _scene(api, cam, dbg, light, resolution, [torus, floor], skymap=p["sky"], **system)
    return _shift(sc, *p["offsets"])


VARIANTS = ("std", "noclip", "f64", "textured", "lh_gl_ortho", "cull_off")


def _adversarial(api, path, variant, resolution, floor=False):
    """A generated mesh under one of VARIANTS: the standard camera; ``Model.clip = False``; float64 vertices
    (``Model @`` a float64 rotation); a ``map_Kd`` texture under the mesh's uv (u from -0.95 to 2.5, v from -1.5 to 1.95:
    _ObjWriter.uv); LH/OpenGL with
    tetra_ortho's orthographic camera; culling off.  (No normal map: upstream's ``inv`` raises on a face without area.)"""
    assert variant in VARIANTS, variant
    system = {}
    if variant == "lh_gl_ortho":
        kw = dict(projection_type=api.PROJECTION_TYPE.ORTHOGRAPHIC, fovy=35, far=20, backface_culling=True)
        cam, dbg = api.Camera((0.5, 1, 2), (0, 0, 0), **kw), api.Camera((0.5, 1, 2), (0, 0, 0), **kw)
        system = dict(system=api.SYSTEM.LH, subsystem=api.SUBSYSTEM.OPENGL)
    else:
        cam, dbg = _std_cameras(api, backface_culling=variant != "cull_off")
    m = api.Model.load_model(path)
    if variant == "noclip":
        m.clip = False
    elif variant == "f64":
        m = m @ (api.rotate_xyz((3.0, -2.0, 1.5)) @ api.scale(1.0))
        assert m.vertices.dtype == np.float64
    elif variant == "textured":
        m.textures.register("diffuse", os.path.join(ASSETS, "grid.tga"), normalize=False)
    models = [m, _floor(api, textured=False)] if floor else [m]
    return _scene(api, cam, dbg, _std_light(api), resolution, models, **system)


def soup(api, seed=0, variant="std", resolution=ADVERSARIAL_RESOLUTION):
    """Triangle soup (soup_obj): sizes from sub-pixel to the whole frame, faces without area, repeats."""
    return _adversarial(api, soup_obj(seed), variant, resolution)


def soup_behind_camera(api, seed=0, variant="std", resolution=ADVERSARIAL_RESOLUTION):
    """The soup after three large faces with corners behind the camera plane (clip-space w < 0).  Upstream writes
    their z and no colour (every fragment fails the ``>= 0`` row filter of obj/triangular.py:139-141); the oracle and
    the kernels shade them.  Parity is defined in front of the camera plane: see DESIGN.md."""
    return _adversarial(api, soup_obj(seed, behind=True), variant, resolution)


def welded(api, seed=0, variant="std", resolution=ADVERSARIAL_RESOLUTION):
    """70 faces on 14 vertices (welded_obj) over the floor that catches their shadow volumes."""
    return _adversarial(api, welded_obj(seed), variant, resolution, floor=True)


def dense_tile(api, seed=0, variant="std", resolution=ADVERSARIAL_RESOLUTION):
    """Hundreds of tiny faces, a coplanar stack and a fan of shadow casters in a few tiles (dense_tile_obj)."""
    return _adversarial(api, dense_tile_obj(seed), variant, resolution)


def face_geometry(scene):
    """Per face of the scene, models in order: clip-space w of its corners (F, 3), whether upstream's cull drops it, and
    its pixel box (x0, x1, y0, y1) as obj/transformation.py:35-43 cuts it (ceil, clamped to the frame; no box -> zeros),
    from the vertices through ``camera.MVP`` and ``camera.viewport``."""
    cam = scene.camera
    h, w = scene.resolution
    ws, culled, boxes = [], [], []
    for model in scene.models:
        corners = np.asarray(model._faces)[:, :, 0]
        clip = np.asarray(model.vertices, dtype=np.float64)[corners] @ cam.MVP              # (F, 3, 4)
        with np.errstate(divide="ignore", invalid="ignore"):
            screen = (clip / clip[..., 3:4]) @ cam.viewport
        n_z = np.cross(screen[:, 1, :3] - screen[:, 0, :3], screen[:, 2, :3] - screen[:, 0, :3])[:, 2]
        lo_x, hi_x = np.maximum(screen[..., 0].min(axis=1), 0), np.minimum(screen[..., 0].max(axis=1), w)
        lo_y, hi_y = np.maximum(screen[..., 1].min(axis=1), 0), np.minimum(screen[..., 1].max(axis=1), h)
        box = np.ceil(np.stack([lo_x, hi_x, lo_y, hi_y], axis=1))
        box[~np.isfinite(box).all(axis=1) | (lo_x > hi_x) | (lo_y > hi_y)] = 0
        ws.append(clip[..., 3]), culled.append(bool(cam.backface_culling) & (n_z < 0)), boxes.append(box.astype(np.int64))
    return np.concatenate(ws), np.concatenate(culled), np.concatenate(boxes)


def behind_camera_pixels(scene, winner):
    """Pixels of a winner map whose face has a corner on or behind the camera plane (clip-space w <= 0)."""
    w, _, _ = face_geometry(scene)
    behind = (w <= 0).any(axis=1)
    return (winner >= 0) & behind[np.maximum(winner, 0)]


# name -> (builder, kwargs); the small ones have full golden buffers committed
SMALL = {
    "cube_small": (cube_small, {}),
    "cube_outward": (cube_outward, {}),
    "diablo_small": (diablo_small, {}),
    "diablo_floor_lh_gl": (diablo_floor_lh_gl, {}),
    "diablo_floor_small": (diablo_floor, {}),
    "torus_spot": (torus_spot, {}),
    "tetra_bare": (tetra_bare, {}),
    "diablo_closeup": (diablo_closeup, {}),
    "cube_skybox": (cube_skybox, {}),
    "torus_skybox_small": (torus_skybox, {"resolution": (216, 384), "nu": 60, "nv": 30}),
    "diablo_nm_object": (diablo_nm_object, {}),
    "diablo_closeup_noclip": (diablo_closeup_noclip, {}),
    "kat_house": (kat_house, {}),
    "tetra_ortho": (tetra_ortho, {}),
    "cube_tetra_nodepth": (cube_tetra_nodepth, {}),
    "gizmos_small": (gizmos_small, {}),
    "fins_nonmanifold": (fins_nonmanifold, {}),
    "wall_nine_materials": (wall_nine_materials, {}),
    "quad_negative_uv": (quad_negative_uv, {}),
    "soup_s0": (soup, {"seed": 0}),
    "welded_s0": (welded, {"seed": 0}),
    "dense_tile_s0": (dense_tile, {"seed": 0}),
    "welded_s4_ortho": (welded, {"seed": 4, "variant": "lh_gl_ortho"}),
    "torus_rect_maps": (torus_rect_maps, {}),
    "quad_rect_object_nm": (quad_rect_object_nm, {}),
    "cube_skybox_offset": (cube_skybox_offset, {}),
    "torus_spot_offset_sky": (torus_spot_offset_sky, {}),
}
# a full capture too, but outside SMALL: its frame is the reference's only in front of the camera plane
BEHIND_CAMERA = {
    "soup_behind_camera_s0": (soup_behind_camera, {"seed": 0}),
}

# BASELINE.json configs at full size: only the uint8 frame, winner map, stencil and z row sums are kept
FULL = {
    "c1_diablo_800x600": (diablo_small, {"resolution": (600, 800)}),       # BASELINE configs[0]; shadows off
    "c2_diablo_1080p": (diablo_small, {"resolution": (1080, 1920)}),       # rendered with shadows off
    "c3_diablo_floor_1080p": (diablo_floor, {"resolution": (1080, 1920)}),
    "c4_torus200k_1080p": (torus_floor, {"resolution": (1080, 1920), "nu": 500, "nv": 200}),
}
# BASELINE.json configs[4]; its capture takes the reference ~8 minutes and is generated separately
HUGE = {
    "c5_torus1m_4k_skybox": (torus_skybox, {"resolution": (2160, 3840), "nu": 1000, "nv": 500}),
}
NO_SHADOW = {"c1_diablo_800x600", "c2_diablo_1080p", "diablo_small_noshadow"}
# the same scenes with upstream's debug-frustum overlay left on (obj/core.py:638)
OVERLAY = ["diablo_small_overlay", "diablo_floor_lh_gl_overlay", "cube_outward_overlay", "torus_spot_offset_sky_overlay"]


def build(api, name):
    if name == "diablo_small_noshadow":
        return diablo_small(api)
    fn, kw = {**SMALL, **BEHIND_CAMERA, **FULL, **HUGE}[name]
    return fn(api, **kw)
