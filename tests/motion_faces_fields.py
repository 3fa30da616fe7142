"""Synthetic inputs for the per-face velocity's kernels and mirrors: hand-made cameras, seeded faces of every awkward kind,
winner maps over a three-model table and a velocity buffer pre-filled with a sentinel pattern.  ``mr_debug_motion_faces_post``
(the device), ``mr_host_face_homographies`` / ``mr_host_velocity_faces`` (the mirrors) and motion_faces_ref.py (NumPy) all
take a ``FaceField``.  tests/test_motion_faces_cpu.py and tests/test_motion_faces_fields_gpu.py share the cases."""
import itertools

import numpy as np

import motion_faces_ref as ref

F32 = np.float32
SIZES = ((1, 1), (1, 40), (37, 1), (33, 65), (45, 70))
FACE_COUNTS = (1, 63, 64, 65, 255, 256, 257)                # wavefront and workgroup edges of k_face_homography
THREE_MODELS = (0, 7, 8)                                    # first faces: seven faces, a model of a single face (7), four faces
THREE_MODELS_FACES = 12
CPU_FLAGS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 0, 0))      # the first, the middle, the last, all, none
ALL_FLAGS = tuple(itertools.product((0, 1), repeat=3))


def camera_s(focal=60.0, centre=(35.0, 22.0), eye=(0.0, 0.0, 0.0), yaw=0.0):
    """The (x, y, w) columns of a perspective camera's world -> un-divided sample grid, 4 x 3, row vectors: a camera at
    *eye* that looks down -z, turned by *yaw* radians round y, with X = focal x + cx w, Y = focal y + cy w, W = w = -z."""
    c, s = np.cos(yaw), np.sin(yaw)
    rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])          # world -> eye, row vectors
    proj = np.array([[focal, 0.0, 0.0], [0.0, focal, 0.0], [-centre[0], -centre[1], -1.0]])
    top = rot @ proj
    return np.vstack([top, -(np.asarray(eye, dtype=np.float64) @ top)[None, :]])


def sentinel(shape):
    """A float32 (H, W, 2) buffer no kernel output equals: NaNs that carry their own index."""
    n = int(np.prod(shape)) * 2
    return (np.uint32(0x7fc00000) + np.arange(n, dtype=np.uint32)).view(F32).reshape(tuple(shape) + (2,))


def bits32(a, b):
    """Floats of *a* whose bits are not *b*'s."""
    return int((np.ascontiguousarray(a, dtype=F32).view(np.uint32) != np.ascontiguousarray(b, dtype=F32).view(np.uint32)).sum())


def bits64(a, b):
    return int((np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) != np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)).sum())


# the awkward faces, by name: where they sit in seeded_faces()'s list
KINDS = ("front", "back", "zero_area", "collinear", "behind_previous", "behind_current", "nan_previous", "sub_sample", "still")


def seeded_faces(n_faces, seed=0):
    """(verts_now, verts_prev (n, 4), corners (n_faces, 3)): the KINDS first (as many as fit), seeded triangles behind
    them.  Three vertices of its own per face; the cameras of ``camera_s()`` see z = -2 .. -6 in front of them."""
    rng = np.random.default_rng(100 + seed)
    now = np.ones((n_faces * 3, 4))
    now[:, 0] = rng.uniform(-1.2, 1.2, n_faces * 3)
    now[:, 1] = rng.uniform(-0.8, 0.8, n_faces * 3)
    now[:, 2] = rng.uniform(-6.0, -2.0, n_faces * 3)
    prev = now.copy()
    prev[:, :3] += rng.uniform(-0.15, 0.15, (n_faces * 3, 3))
    corners = np.arange(n_faces * 3).reshape(n_faces, 3)

    def tri(f, pts):
        now[f * 3:f * 3 + 3, :3] = pts
        prev[f * 3:f * 3 + 3, :3] = np.asarray(pts) + (0.1, -0.05, 0.02)

    for f, kind in enumerate(KINDS[:n_faces]):
        if kind == "front":
            tri(f, [(-0.5, -0.4, -3.0), (0.6, -0.3, -3.5), (0.0, 0.5, -2.5)])
        elif kind == "back":
            tri(f, [(-0.5, -0.4, -3.0), (0.0, 0.5, -2.5), (0.6, -0.3, -3.5)])
        elif kind == "zero_area":
            tri(f, [(0.1, 0.1, -3.0), (0.1, 0.1, -3.0), (0.4, 0.2, -3.0)])
        elif kind == "collinear":
            tri(f, [(-0.5, -0.5, -4.0), (0.0, 0.0, -4.0), (0.25, 0.25, -4.0)])
        elif kind == "behind_previous":
            tri(f, [(-0.5, -0.4, -3.0), (0.6, -0.3, -3.5), (0.0, 0.5, -2.5)])
            prev[f * 3, 2] = 1.5                                     # that corner lay behind the previous camera
        elif kind == "behind_current":
            tri(f, [(-0.5, -0.4, -3.0), (0.6, -0.3, 0.75), (0.0, 0.5, -2.5)])
        elif kind == "nan_previous":
            tri(f, [(-0.3, -0.2, -3.0), (0.4, -0.1, -3.2), (0.1, 0.4, -2.8)])
            prev[f * 3 + 1, 1] = np.nan
        elif kind == "sub_sample":
            tri(f, [(0.001, 0.001, -3.0), (0.004, 0.001, -3.0), (0.002, 0.005, -3.0)])
        elif kind == "still":
            tri(f, [(-0.2, -0.6, -5.0), (0.7, -0.5, -5.5), (0.2, 0.3, -4.5)])
            prev[f * 3:f * 3 + 3] = now[f * 3:f * 3 + 3]
    return now, prev, corners


def winner_map(shape, n_faces, face_off, seed=0):
    """Winners of every kind: -1, the first and the last face of every model, and seeded faces of the whole range."""
    rng = np.random.default_rng(200 + seed)
    face_off = list(face_off)
    ends = face_off[1:] + [n_faces]
    special = [-1] + [f for a, b in zip(face_off, ends) if b > a for f in (a, b - 1)]
    winner = rng.integers(-1, n_faces, shape).astype(np.int32)
    pick = rng.random(shape) < 0.3
    winner[pick] = np.asarray(special, dtype=np.int32)[rng.integers(0, len(special), int(pick.sum()))]
    flat = winner.ravel()
    flat[:len(special)] = special[:flat.size]                         # (each at least once where the map has room)
    return winner


class FaceField:
    """One frame's inputs for the two kernels."""

    def __init__(self, name, verts_now, verts_prev, corners, face_off, deforming, s_now, s_prev, winner, velocity=None):
        self.name = name
        self.verts_now = np.ascontiguousarray(verts_now, dtype=np.float64)
        self.verts_prev = np.ascontiguousarray(verts_prev, dtype=np.float64)
        self.corners = np.ascontiguousarray(corners, dtype=np.int32).reshape(-1, 3)
        self.face_off = np.asarray(face_off, dtype=np.int32)
        self.deforming = np.asarray(deforming, dtype=np.int32)
        self.s_now, self.s_prev = np.ascontiguousarray(s_now, dtype=np.float64), np.ascontiguousarray(s_prev, dtype=np.float64)
        self.winner = np.ascontiguousarray(winner, dtype=np.int32)
        self.velocity = sentinel(self.winner.shape) if velocity is None else np.ascontiguousarray(velocity, dtype=F32)
        assert len(self.face_off) == len(self.deforming) and self.velocity.shape == self.winner.shape + (2,)

    def __repr__(self):
        return f"FaceField({self.name!r}, {len(self.corners)} faces, {self.winner.shape}, flags {self.deforming.tolist()})"

    def layout(self):
        """(hom_off, the flagged faces in record order) as the library lays the records out."""
        ends = np.append(self.face_off[1:], len(self.corners))
        hom_off, faces = np.full(len(self.face_off), -1, dtype=np.int32), []
        for m, flagged in enumerate(self.deforming):
            if flagged and ends[m] > self.face_off[m]:
                hom_off[m] = len(faces)
                faces.extend(range(self.face_off[m], ends[m]))
        return hom_off, np.asarray(faces, dtype=np.int64)

    def touched(self):
        """The samples the pass overwrites: covered, and their model flagged."""
        import motion_ref
        covered = self.winner >= 0
        model = np.zeros(self.winner.shape, dtype=np.int64)
        model[covered] = motion_ref.model_of(self.face_off, self.winner[covered])
        return covered & (self.deforming[model] != 0)

    def reference(self):
        hom_off, faces = self.layout()
        H = ref.homographies(self.verts_now, self.verts_prev, self.corners[faces], self.s_now, self.s_prev)
        return H, ref.velocity_faces(self.winner, self.face_off, hom_off, H, self.velocity)

    def mirror(self, native):
        hom_off, faces = self.layout()
        H = native.host_face_homographies(self.verts_now, self.verts_prev, native.face_records(self.corners[faces]), self.s_now, self.s_prev)
        return H, native.host_velocity_faces(self.winner, self.face_off, hom_off, H, self.velocity)

    def device(self, native, handle):
        return native.debug_motion_faces_post(handle, self.verts_now, self.verts_prev, native.face_records(self.corners), self.face_off,
                                              self.deforming, self.s_now, self.s_prev, self.winner, self.velocity)


def three_models(shape, flags, seed=0, s_now=None, s_prev=None):
    """The KINDS and three seeded faces over the three-model table, a winner map of *shape*, these flags."""
    now, prev, corners = seeded_faces(THREE_MODELS_FACES, seed)
    s_now = camera_s() if s_now is None else s_now
    s_prev = camera_s(eye=(0.05, -0.02, 0.1), yaw=0.01) if s_prev is None else s_prev
    return FaceField(f"three{tuple(flags)}", now, prev, corners, THREE_MODELS, flags, s_now, s_prev,
                     winner_map(shape, THREE_MODELS_FACES, THREE_MODELS, seed))


def counted(n_faces, shape=(33, 65), seed=0):
    """One flagged model of *n_faces* faces (the KINDS first), every face a winner somewhere."""
    now, prev, corners = seeded_faces(n_faces, seed)
    return FaceField(f"count{n_faces}", now, prev, corners, (0,), (1,), camera_s(), camera_s(eye=(0.05, -0.02, 0.1), yaw=0.01),
                     winner_map(shape, n_faces, (0,), seed))
