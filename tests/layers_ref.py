"""The data layers' definition (csrc/layers_def.h) restated twice: in NumPy, operation for operation, so that the host
mirror can be held to it bit for bit; and over ``fractions.Fraction``, exactly, with the absolute-value evaluations the
error bound of layers_def.h is made of.  And the mutants a test must tell apart from the definition.

Face records are the arrays ``_native.host_layers`` takes: ``pos`` with fields v (n, 3, 4), material, flags; ``attr`` with
fields uv (n, 3, 2) and n (n, 3, 3).  ``S`` is float64 (4, 4), row vectors: columns x, y, w, e."""
from fractions import Fraction

import numpy as np

NAMES = ("model", "face", "material", "barycentric", "depth", "position", "face_normal", "normal", "uv")
CHANNELS = dict(zip(NAMES, (1, 1, 1, 3, 1, 3, 3, 3, 2)))
FF_HAS_NORMALS, FF_HAS_UV = 4, 8
MUTANTS = ("unjittered", "screen_linear", "w_as_depth", "winding", "unnormalised", "face_global", "boundary")


def model_of(face_off, w, mutant=None):
    """The last m with face_off[m] <= w.  The ``boundary`` mutant compares with < instead."""
    return np.searchsorted(np.asarray(face_off), w, side="left" if mutant == "boundary" else "right") - 1


def _cross(a, b):
    """(..., 3) x (..., 3), each component a*b - c*d."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _blend(lam, a):
    """(lam_0 a_0 + lam_1 a_1) + lam_2 a_2 over samples: lam (n, 3), a (n, 3, c)."""
    return (lam[:, 0, None] * a[:, 0] + lam[:, 1, None] * a[:, 1]) + lam[:, 2, None] * a[:, 2]


def layers(winner, pos, attr, face_off, S, mutant=None, S_plain=None):
    """Every layer as a dict name -> array, and the boolean map of degenerate samples.  *mutant*: one of ``MUTANTS``
    (``unjittered`` uses *S_plain* in place of *S*)."""
    winner = np.asarray(winner, dtype=np.int32)
    h, w_ = winner.shape
    S = np.asarray(S_plain if mutant == "unjittered" else S, dtype=np.float64)
    out = {name: np.zeros((h, w_) + ((CHANNELS[name],) if CHANNELS[name] > 1 else ()), np.int32 if name in NAMES[:3] else np.float32)
           for name in NAMES}
    for name in NAMES[:3]:
        out[name][...] = -1
    out["depth"][...] = np.inf
    degenerate = np.zeros((h, w_), dtype=bool)
    ys, xs = np.nonzero(winner >= 0)
    if len(ys) == 0:
        return out, degenerate
    w = winner[ys, xs]
    model = model_of(face_off, w, mutant)
    out["model"][ys, xs] = model
    out["face"][ys, xs] = w if mutant == "face_global" else w - np.asarray(face_off)[np.maximum(model, 0)]
    out["material"][ys, xs] = pos["material"][w]
    with np.errstate(all="ignore"):
        V = pos["v"][w][:, :, :3].astype(np.float64)                                      # (n, 3 corners, 3)
        c = ((V[:, :, 0, None] * S[0] + V[:, :, 1, None] * S[1]) + V[:, :, 2, None] * S[2]) + S[3]      # (n, 3 corners, 4)
        X, Y, W, E = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
        A = np.stack([_cross(Y, W), _cross(W, X), _cross(X, Y)], axis=1)                  # (n, 3, 3)
        xd, yd = xs.astype(np.float64)[:, None], ys.astype(np.float64)[:, None]
        if mutant == "screen_linear":
            px, py = X / W, Y / W                                                         # barycentrics of the projected triangle
            A = np.stack([np.stack([py[:, 1] - py[:, 2], py[:, 2] - py[:, 0], py[:, 0] - py[:, 1]], -1),
                          np.stack([px[:, 2] - px[:, 1], px[:, 0] - px[:, 2], px[:, 1] - px[:, 0]], -1),
                          np.stack([px[:, 1] * py[:, 2] - px[:, 2] * py[:, 1], px[:, 2] * py[:, 0] - px[:, 0] * py[:, 2],
                                    px[:, 0] * py[:, 1] - px[:, 1] * py[:, 0]], -1)], axis=1)
        b = (xd * A[:, 0] + yd * A[:, 1]) + A[:, 2]
        sigma = (b[:, 0] + b[:, 1]) + b[:, 2]
        lam = b / sigma[:, None]
        bad = ~(np.isfinite(sigma) & (sigma != 0) & np.isfinite(lam).all(axis=1))
        depth = (lam[:, 0] * E[:, 0] + lam[:, 1] * E[:, 1]) + lam[:, 2] * E[:, 2]
        if mutant == "w_as_depth":
            depth = (lam[:, 0] * W[:, 0] + lam[:, 1] * W[:, 1]) + lam[:, 2] * W[:, 2]
        position = _blend(lam, V)
        p, q = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
        g = _cross(q, p) if mutant == "winding" else _cross(p, q)
        l = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = np.isfinite(l) & (l > 0)
        face_normal = np.where(ok[:, None], (g / l[:, None]).astype(np.float32), np.float32(0))
        flags = pos["flags"][w]
        m = _blend(lam, attr["n"][w].astype(np.float64))
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        own = ((flags & FF_HAS_NORMALS) != 0) & np.isfinite(length) & (length > 0)
        blended = m if mutant == "unnormalised" else m / length[:, None]
        normal = np.where(own[:, None], blended.astype(np.float32), face_normal)
        uv = np.where(((flags & FF_HAS_UV) != 0)[:, None], _blend(lam, attr["uv"][w].astype(np.float64)).astype(np.float32), np.float32(0))
        fields = {"barycentric": lam.astype(np.float32), "depth": depth.astype(np.float32), "position": position.astype(np.float32),
                  "face_normal": face_normal, "normal": normal, "uv": uv}
    good = ~bad
    for name, value in fields.items():
        out[name][ys[good], xs[good]] = value[good]
    degenerate[ys[bad], xs[bad]] = True
    return out, degenerate


def _frac(a):
    return [Fraction(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()]


def exact_sample(V, uv, S, x, y):
    """One sample over Fractions.  *V* (3, 3), *uv* (3, 2), *S* (4, 4): finite floats.  Returns ``None`` where sigma == 0, else a
    dict with the exact ``lam`` (3), ``depth``, ``position`` (3), ``uv`` (2) and what the error bound of layers_def.h reads:
    ``kappa`` (3), ``ratio`` = bar(sigma) / |sigma|, ``E`` and ``barE`` (3 each: the corners' eye depths and their
    absolute-value evaluations)."""
    V = [_frac(row) for row in np.asarray(V)]
    S = [_frac(row) for row in np.asarray(S)]
    c = [[V[k][0] * S[0][j] + V[k][1] * S[1][j] + V[k][2] * S[2][j] + S[3][j] for j in range(4)] for k in range(3)]
    cbar = [[abs(V[k][0] * S[0][j]) + abs(V[k][1] * S[1][j]) + abs(V[k][2] * S[2][j]) + abs(S[3][j]) for j in range(4)] for k in range(3)]
    col = lambda t, j: [t[k][j] for k in range(3)]
    X, Y, W = col(c, 0), col(c, 1), col(c, 2)
    Xb, Yb, Wb = col(cbar, 0), col(cbar, 1), col(cbar, 2)
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    cross_bar = lambda a, b: [a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]]
    A = [cross(Y, W), cross(W, X), cross(X, Y)]
    Abar = [cross_bar(Yb, Wb), cross_bar(Wb, Xb), cross_bar(Xb, Yb)]
    bk = [x * A[0][k] + y * A[1][k] + A[2][k] for k in range(3)]
    bbar = [abs(x) * Abar[0][k] + abs(y) * Abar[1][k] + Abar[2][k] for k in range(3)]
    sigma, sbar = sum(bk), sum(bbar)
    if sigma == 0:
        return None
    lam = [v / sigma for v in bk]
    uvf = [_frac(row) for row in np.asarray(uv)]
    return {"lam": lam,
            "depth": sum(lam[k] * c[k][3] for k in range(3)),
            "position": [sum(lam[k] * V[k][j] for k in range(3)) for j in range(3)],
            "uv": [sum(lam[k] * uvf[k][j] for k in range(3)) for j in range(2)],
            "kappa": [(bbar[k] + abs(lam[k]) * sbar) / abs(sigma) for k in range(3)],
            "ratio": sbar / abs(sigma),
            "E": [c[k][3] for k in range(3)], "barE": [cbar[k][3] for k in range(3)],
            "V": V, "uv_corners": uvf}


U = Fraction(1, 2 ** 53)


def bounds(e):
    """The error bounds of layers_def.h for one ``exact_sample``: a dict with ``lam`` (3), ``depth``, ``position`` (3), ``uv``
    (2) as Fractions, each including the final rounding to float32; ``None`` where the sample has no bound
    (16 u bar(sigma) / |sigma| > 1/2)."""
    if 16 * U * e["ratio"] > Fraction(1, 2):
        return None
    E = [32 * U * k for k in e["kappa"]]
    lam = e["lam"]

    def with_f32(t, err):
        """err, the float64 result's distance from t, and the rounding of that result to float32"""
        return err + max((abs(t) + err) * Fraction(1, 2 ** 24), Fraction(1, 2 ** 149))

    def blend(a, d, t):
        first = sum(E[k] * abs(a[k]) + abs(lam[k]) * d[k] for k in range(3))
        return with_f32(t, first + 4 * U * sum((abs(lam[k]) + E[k]) * (abs(a[k]) + d[k]) for k in range(3)))
    gamma4 = Fraction(101, 100) * 4 * U
    zero = [Fraction(0)] * 3
    return {"lam": [with_f32(lam[k], E[k]) for k in range(3)],
            "depth": blend(e["E"], [gamma4 * b for b in e["barE"]], e["depth"]),
            "position": [blend([e["V"][k][j] for k in range(3)], zero, e["position"][j]) for j in range(3)],
            "uv": [blend([e["uv_corners"][k][j] for k in range(3)], zero, e["uv"][j]) for j in range(2)]}
