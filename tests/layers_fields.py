"""Synthetic fields for the data layers: hand-made cameras, a three-model face table with an empty model in the middle,
faces of every awkward kind in both record types, and small winner maps whose widths are no multiple of the workgroup.

A sample need not lie inside its winner face: the definition lives on the face's plane, and the winner maps here put every
face under samples all over the grid."""
import numpy as np

from py_numpy_renderer_amd import _native

FF_HAS_NORMALS, FF_HAS_UV = 4, 8
SHAPES = ((1, 1), (1, 256), (3, 257), (5, 67))          # (rows, columns): a block edge inside a row, and rows that straddle one
JITTER = (0.25, -0.375)                                  # dyadic, in samples


def camera(kind, jitter=(0.0, 0.0)):
    """S (4, 4) float64, row vectors, columns x, y, w, e, with dyadic entries.  The eye sits at (1/4, -1/2, 6) and looks down
    -z (``rh``, ``ortho``) or sits at (1/4, -1/2, -6) and looks down +z (``lh``); 32 samples a world unit at distance 1
    (perspective) or everywhere (orthographic); the grid's centre at (33.5, 2.5) plus the jitter."""
    cx, cy = 33.5 + jitter[0], 2.5 + jitter[1]
    a = 32.0
    S = np.zeros((4, 4))
    if kind == "ortho":
        eye = np.array([0.25, -0.5, 6.0])
        S[0, 0] = a; S[1, 1] = a; S[3, 0] = cx - a * eye[0]; S[3, 1] = cy - a * eye[1]
        S[3, 2] = 1.0
        S[2, 3] = -1.0; S[3, 3] = eye[2]                 # e = -(z - eye.z)
        return S
    sign = -1.0 if kind == "rh" else 1.0                 # w = sign * (z - eye.z)
    eye = np.array([0.25, -0.5, 6.0 if kind == "rh" else -6.0])
    wcol = np.array([0.0, 0.0, sign, -sign * eye[2]])
    S[:, 2] = wcol
    S[:, 3] = wcol
    S[:, 0] = cx * wcol; S[0, 0] += a; S[3, 0] -= a * eye[0]
    S[:, 1] = cy * wcol; S[1, 1] += a; S[3, 1] -= a * eye[1]
    return S


def seeded_camera(seed):
    """A camera whose entries are not dyadic: ``camera('rh')`` times a small seeded perturbation."""
    rng = np.random.default_rng(seed)
    return camera("rh", JITTER) * (1.0 + 0.01 * rng.standard_normal((4, 4)))


CAMERAS = ("rh", "lh", "ortho")

# the kinds of the faces, in the order every model lists them
KINDS = ("dyadic", "dyadic_tilted", "seeded", "sliver", "zero_area", "straddling", "nan_vertex", "no_normals", "no_uv", "cancelling", "seeded_far")
DEGENERATE_KINDS = ("zero_area", "nan_vertex")


def _face(kind, rng, z_sign):
    """(corners (3, 3), flags, uv (3, 2), normals (3, 3)) of one face; z_sign = +1 puts it in front of the rh / ortho cameras."""
    dy = lambda *shape: np.round(rng.uniform(-3, 3, shape) * 8) / 8
    flags = FF_HAS_NORMALS | FF_HAS_UV
    uv = np.round(rng.uniform(0, 1, (3, 2)) * 64) / 64 if kind.startswith("dyadic") else rng.uniform(0, 1, (3, 2))
    normals = rng.standard_normal((3, 3))
    if kind == "dyadic":
        # a right triangle with legs 2 and 1 at w = 4 (or under the orthographic camera): sigma is 2048 at every sample, a
        # power of two, so every lambda, and every sum of products with dyadic corners, is exact in float64
        v = np.array([[0.0, 0.0, 2.0], [2.0, 0.0, 2.0], [0.0, 1.0, 2.0]]) + np.array([dy(), dy(), 0.0])
        normals = np.array([[0.0, 0.0, 1.0], [0.0, 0.6, 0.8], [0.6, 0.0, 0.8]])
    elif kind == "dyadic_tilted":
        v = np.array([[-2.0, -1.0, -1.5], [2.5, -1.5, 1.0], [0.25, 2.0, 2.5]])
        normals = np.array([[0.0, 0.0, 2.0], [0.0, 3.0, 4.0], [0.5, 0.0, 0.5]])
    elif kind == "seeded":
        v = rng.uniform(-3, 3, (3, 3))
    elif kind == "seeded_far":
        v = rng.uniform(-3, 3, (3, 3)) + np.array([0.0, 0.0, -40.0])
    elif kind == "sliver":
        a, b = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
        v = np.array([a, b, a + (b - a) * 0.37 + rng.standard_normal(3) * 1e-6])
    elif kind == "zero_area":
        a, d = np.array([-1.5, 0.5, 0.25]), np.array([0.5, 0.25, -0.125])
        v = np.array([a, a + 2 * d, a + 5 * d])
    elif kind == "straddling":
        v = np.array([[-2.0, -1.0, 2.0], [2.0, -1.0, 2.0], [0.0, 1.0, 9.5]])                # the third corner behind the camera plane
    elif kind == "nan_vertex":
        v = dy(3, 3)
        v[1, 1] = np.nan
    elif kind == "no_normals":
        v, flags = dy(3, 3) + np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0]]), FF_HAS_UV
    elif kind == "no_uv":
        v, flags = dy(3, 3) + np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0]]), FF_HAS_NORMALS
    elif kind == "cancelling":
        v = dy(3, 3) + np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0]])
        normals = np.zeros((3, 3))
    else:
        raise ValueError(kind)
    v = v.copy()
    v[:, 2] *= z_sign
    return v, flags, uv, normals


class Field:
    """One case: records, table, winner map, cameras.  ``kinds[f]`` names face f's kind."""

    def __init__(self, name, pos32, shape, seed, lh=False, dyadic_only=True):
        rng = np.random.default_rng(seed)
        self.name, self.pos32, self.shape, self.lh = name, pos32, shape, lh
        n0, n2 = len(KINDS), len(KINDS)
        self.kinds = KINDS + KINDS
        self.face_off = np.array([0, n0, n0], dtype=np.int32)                              # the model in the middle is empty
        n = n0 + n2
        self.pos = np.zeros(n, dtype=_native.FACE_POS_DTYPES[bool(pos32)])
        self.attr = np.zeros(n, dtype=_native.FACE_ATTR_DTYPE)
        for f, kind in enumerate(self.kinds):
            v, flags, uv, normals = _face(kind, rng, -1.0 if lh else 1.0)
            self.pos["v"][f, :, :3] = v
            self.pos["v"][f, :, 3] = 1.0
            self.pos["material"][f] = 7 + 3 * f
            self.pos["flags"][f] = flags | 1                                               # (FF_CLIP: a flag the layers do not read)
            self.attr["uv"][f], self.attr["n"][f] = uv, normals
        self.pos["pad"][...] = 0xdeadbeef                                                  # (never read)
        self.attr["pad"][...] = np.nan
        h, w = shape
        faces = np.arange(n)
        winner = rng.choice(np.concatenate([faces, [-1, -1, -1]]), size=(h, w)).astype(np.int32)
        # -1 samples and the first and last face of every model at the start of the map and round every block edge
        forced = [-1, 0, n0 - 1, n0, n - 1]
        flat = winner.ravel()
        for edge in range(0, flat.size, 256):
            for k, value in enumerate(forced):
                for at in (edge + k, edge - 1 - k):
                    if 0 <= at < flat.size:
                        flat[at] = value
        if flat.size == 1:
            flat[0] = seed % n
        self.winner = flat.reshape(h, w)

    def without(self, kinds):
        """A copy of the winner map with the samples of these kinds of face set to -1."""
        drop = np.array([k in kinds for k in self.kinds])
        w = self.winner.copy()
        w[(w >= 0) & drop[np.maximum(w, 0)]] = -1
        return w

    def camera(self, kind=None, jitter=JITTER):
        return camera(kind or ("lh" if self.lh else "rh"), jitter)

    def desc(self, S, mask=0x1ff):
        return _native.fill_layers_desc(S, mask, len(self.face_off))

    def degenerate_samples(self, winner=None):
        w = self.winner if winner is None else winner
        bad = np.array([k in DEGENERATE_KINDS for k in self.kinds])
        return int(((w >= 0) & bad[np.maximum(w, 0)]).sum())

    def __repr__(self):
        return f"Field({self.name})"


def fields():
    out = []
    for i, shape in enumerate(SHAPES):
        for pos32 in (True, False):
            for lh in (False, True):
                name = f"{shape[0]}x{shape[1]}-{'pos32' if pos32 else 'pos64'}-{'lh' if lh else 'rh'}"
                out.append(Field(name, pos32, shape, 100 + 10 * i + 2 * pos32 + lh, lh=lh))
    return out


def same_bits(a, b):
    """The number of 32-bit words in which two arrays of one 4-byte dtype differ."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.dtype.itemsize == 4, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())
