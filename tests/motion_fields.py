"""Synthetic inputs for the motion blur's kernels and mirrors: z-buffers, winner maps, colours and hand-made class matrices
that no camera produces.  ``mr_debug_motion_post`` (the device), ``mr_host_velocity`` / ``mr_host_motion_blur`` (the
mirrors) and motion_ref.py (NumPy) all take a ``Field``.  tests/test_motion_cpu.py and tests/test_motion_fields_gpu.py
share the cases; the depth fields and the Moebius map are post_fields.py's."""
import numpy as np

import motion_ref
import post_fields

F32 = np.float32
MOEBIUS, IDENTITY = post_fields.MOEBIUS, post_fields.IDENTITY

# workgroup shapes as mr_debug_motion_post numbers them (csrc/motion.hip): samples per side; 0 and 1 differ in the threads
MBLUR_TILES = (32, 32, 16)
CPU_SIZES = ((1, 1), (1, 40), (37, 1), (33, 65), (45, 70))      # the last: no multiple of any shape, more than one 32 x 32 both ways
GPU_SIZES = ((1, 1), (3, 200), (200, 3), (64, 64), (45, 70))
COMPASS = tuple((float(np.cos(k * np.pi / 4)), float(np.sin(k * np.pi / 4))) for k in range(8))

IDENTITY_T = np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]])
IDENTITY_B = np.eye(3)
THREE_MODELS = (0, 7, 8)                         # first faces: seven faces, a model of a single face (7), four faces
THREE_MODELS_FACES = 12


def shift_t(ux, uy):
    """The class matrix under which every sample has moved by (ux, uy): it was at (x - ux, y - uy)."""
    t = IDENTITY_T.copy()
    t[2, 0], t[2, 1] = -ux, -uy
    return t


def shift_b(ux, uy):
    b = IDENTITY_B.copy()
    b[2, 0], b[2, 1] = -ux, -uy
    return b


class Field:
    """One frame for the two kernels."""

    def __init__(self, name, z, winner, frame, face_off=(), matrices=(IDENTITY_T,), background=IDENTITY_B, class_of_model=(),
                 m=MOEBIUS, shutter=1.0):
        self.name = name
        self.z = np.ascontiguousarray(z, dtype=np.float64)
        self.winner = np.ascontiguousarray(winner, dtype=np.int32)
        self.frame = np.ascontiguousarray(frame, dtype=F32)
        self.face_off = np.asarray(face_off, dtype=np.int32)
        self.matrices = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 4, 3)
        self.background = np.ascontiguousarray(background, dtype=np.float64)
        self.class_of_model = np.asarray(class_of_model, dtype=np.int32)
        self.m, self.shutter = tuple(m), float(shutter)
        assert self.winner.shape == self.z.shape and self.frame.shape == self.z.shape + (3,)
        assert len(self.face_off) == len(self.class_of_model)

    @property
    def shape(self):
        return self.z.shape

    def __repr__(self):
        return f"Field({self.name!r}, {self.shape})"

    def desc(self, native):
        return native.fill_motion_desc(self.m, self.shutter, self.matrices, self.background, self.class_of_model)

    def reference(self):
        return motion_ref.apply(self.z, self.winner, self.frame, self.face_off, self.m, self.shutter, self.matrices, self.background,
                                self.class_of_model)

    def mirror(self, native):
        d = self.desc(native)
        u = native.host_velocity(self.z, self.winner, self.face_off, d)
        return u, native.host_motion_blur(self.z, u, self.frame, d)

    def device(self, native, handle, shape=0):
        return native.debug_motion_post(handle, self.z, self.winner, self.frame, self.face_off, self.desc(native), shape)


def bits(a, b):
    """Floats of *a* whose bits are not *b*'s."""
    return int((np.ascontiguousarray(a, dtype=F32).view(np.uint32) != np.ascontiguousarray(b, dtype=F32).view(np.uint32)).sum())


def plane(shape, seed, depth=2.0):
    """(Z, winner, F): one face at constant eye depth under MOEBIUS, seeded colours."""
    z = np.full(shape, post_fields.z_of(depth, MOEBIUS))
    return z, np.zeros(shape, dtype=np.int32), np.random.default_rng(seed).random(tuple(shape) + (3,), dtype=np.float32)


def hills(shape, seed):
    """(Z, winner, F): post_fields.dof_hills -- steps in depth, holes of +inf, -inf and NaN -- with winner -1 in the holes."""
    z, frame = post_fields.dof_hills(shape, seed)
    return z, np.where(np.isfinite(z), 0, -1).astype(np.int32), frame


def at_rest(shape, seed=1):
    z, winner, frame = hills(shape, seed)
    return Field("rest", z, winner, frame, face_off=(0,), class_of_model=(0,))


def uniform(shape, u, seed=2, shutter=1.0, name=None):
    """Every sample, the holes' background too, moved by *u*."""
    z, winner, frame = hills(shape, seed)
    return Field(name or f"uniform{u}", z, winner, frame, face_off=(0,), class_of_model=(0,), matrices=(shift_t(*u),),
                 background=shift_b(*u), shutter=shutter)


def clamped(shape, direction, seed=3):
    """A uniform field at the 16-sample clamp: 40 samples along *direction*."""
    return uniform(shape, (40.0 * direction[0], 40.0 * direction[1]), seed, name=f"clamp{direction}")


def patches(shape, seed=4):
    """Sixteen seeded directions and lengths (0 .. 36 samples: at rest, short, long, beyond the clamp) in patches of 16 x
    16 samples, so the seams lie on columns 15/16, 31/32 ... and on the same rows: on workgroup boundaries.  Every patch is
    a model of its own with a class of its own; the depths step from patch to patch, so `behind` is met both ways."""
    rng = np.random.default_rng(seed)
    h, w = shape
    ys, xs = np.mgrid[0:h, 0:w]
    patch = ((ys // 16) % 4) * 4 + (xs // 16) % 4
    lengths = np.concatenate(([0.0, 0.6, 0.99, 1.01], rng.uniform(1.5, 36.0, 12)))
    angles = rng.uniform(0, 2 * np.pi, 16)
    order = rng.permutation(16)
    matrices = [IDENTITY_T] + [shift_t(lengths[k] * np.cos(angles[k]), lengths[k] * np.sin(angles[k])) for k in order]
    depth = 1.5 + 0.25 * rng.permutation(16)[patch] + 0.01 * rng.random(shape)
    z = post_fields.z_of(depth, MOEBIUS)
    frame = rng.random((h, w, 3), dtype=np.float32)
    face_off = np.arange(16) * 3                                     # three faces a model
    winner = (patch * 3 + rng.integers(0, 3, shape)).astype(np.int32)
    return Field("patches", z, winner, frame, face_off=face_off, class_of_model=np.arange(1, 17), matrices=matrices)


def owners(shape, seed=5):
    """The winner map's corners: -1 on finite Z (class 0), the first and the last face of every model of THREE_MODELS, the
    model of a single face; Z with +inf, -inf and NaN under winners of every kind (they are background whatever the winner
    says).  Model 0 is at rest in class 0, models 1 and 2 have classes of their own; the background moves too."""
    rng = np.random.default_rng(seed)
    z, _, frame = hills(shape, seed)
    choice = np.array([-1, 0, 6, 7, 8, 11], dtype=np.int32)
    winner = choice[rng.integers(0, len(choice), shape)]
    return Field("owners", z, winner, frame, face_off=THREE_MODELS, class_of_model=(0, 2, 1),
                 matrices=(IDENTITY_T, shift_t(5.0, -3.0), shift_t(-9.5, 0.25)), background=shift_b(0.0, 7.0))


def behind_camera(shape, seed=6):
    """A class whose third component falls to zero and below across the frame: u_2 = Z (1 - x / 20.5), so the samples from
    column 21 on lay behind the previous camera and U must be 0 there; in front of that the motion grows towards the pole."""
    z, winner, frame = plane(shape, seed)
    t = shift_t(2.0, 1.0)
    t[0, 2] = -1.0 / 20.5
    return Field("behind", z, winner, frame, face_off=(0,), class_of_model=(1,), matrices=(IDENTITY_T, t))


def gpu_cases(shape):
    """Every field the kernels are shown at one size."""
    return ([at_rest(shape)] + [clamped(shape, d) for d in COMPASS] + [patches(shape), owners(shape), behind_camera(shape),
            uniform(shape, (6.0, 2.5), shutter=0.5, name="half_shutter")])


def h_max(field, tile, halo=True):
    """The largest half-length among the samples each workgroup of *tile* x *tile* samples stages (its rectangle and, with
    *halo*, 16 samples round it), as a (rows, cols) array: motion_bound of it is the workgroup's loop bound."""
    u = motion_ref.velocity(field.z, field.winner, field.face_off, field.matrices, field.background, field.class_of_model)
    h = motion_ref.segment(u, field.shutter)[0]
    rows, cols = -(-h.shape[0] // tile), -(-h.shape[1] // tile)
    r = 16 if halo else 0
    out = np.zeros((rows, cols), dtype=F32)
    for j in range(rows):
        for i in range(cols):
            out[j, i] = h[max(0, j * tile - r):(j + 1) * tile + r, max(0, i * tile - r):(i + 1) * tile + r].max()
    return out


def bound_of(h):
    """motion_bound (csrc/motion_def.h)."""
    return 0 if not h > 0 else min(int(F32(h) + F32(1)), 16)
