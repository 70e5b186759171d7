"""Test helper: a numpy float64 restatement of the mesh -> SDF rule of the reference's brute-force kernels
(wisp/csrc/external/mesh2sdf_kernel.cu:334-583 distance and stabbing tests, :585-840 nearest triangle, :844-970 aggregation), with
the reference's float roundings and an ambiguity mask for the sign, plus procedural mesh builders.  Product code never imports it.

Rule per point p over triangles (a, b, c): edges e10 = b - a, e21 = c - b, e02 = a - c, normal n = e10 x e02; triangles with n == 0
are skipped for the distance.  Face case iff (e_k x n) . (p - v_k) has no sign bit set for all three edges: distsq = (n . (p - a))^2
r_n; else distsq = min_k |e_k c_k - (p - v_k)|^2 with c_k = clamp_f32(f32(e_k . (p - v_k) r_k), 0, 1).  r = f32(1 / f32(|x|^2)).
distsq is rounded to float per triangle; |sdf| = f32(sqrt(min)).  Sign: 13 directions d; for each triangle (degenerate ones
included) and d: pvec = d x e2 (e2 = c - a), det = e10 . pvec, skipped if |det| < 1e-8; u = (p - a) . pvec / det in [0, 1],
q = (p - a) x e10, v = d . q / det >= 0, u + v <= 1, t = e2 . q / det sets the 'positive' (t >= 0) or 'negative' bit of d.  Inside
(sdf < 0) iff both bits of all 13 directions are set."""
import numpy as np

C2 = float(np.float32(0.707106781))
C3 = float(np.float32(0.577350269))
DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1],
                 [0, C2, C2], [C2, 0, C2], [C2, C2, 0],
                 [0, C2, -C2], [C2, 0, -C2], [C2, -C2, 0],
                 [C3, C3, C3], [-C3, C3, C3], [C3, -C3, C3], [C3, C3, -C3]], dtype=np.float64)
DET_EPS = 1e-8
AMBIGUITY = 1e-9
EPS64 = np.finfo(np.float64).eps


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def frcp(x):
    """__frcp_rn(float(x)) as a double."""
    with np.errstate(divide='ignore'):
        return f32(1.0 / f32(x))


def _dot(a, b):
    return (a * b).sum(-1)


class Prepared:
    """Per-triangle quantities of T [F,3,3] (float64)."""

    def __init__(self, T):
        T = np.asarray(T, dtype=np.float64)
        self.a, self.b, self.c = T[:, 0], T[:, 1], T[:, 2]
        self.e10, self.e21, self.e02 = self.b - self.a, self.c - self.b, self.a - self.c
        self.n = np.cross(self.e10, self.e02)
        self.cn = [np.cross(e, self.n) for e in (self.e10, self.e21, self.e02)]
        self.r = [frcp(_dot(e, e)) for e in (self.e10, self.e21, self.e02)]
        self.rn = frcp(_dot(self.n, self.n))
        self.degenerate = ~np.any(self.n != 0.0, axis=1)
        self.e2 = -self.e02
        self.pvec = np.cross(DIRS[None, :, :], self.e2[:, None, :])            # [F,13,3]
        self.det = _dot(self.e10[:, None, :], self.pvec)                       # [F,13]
        self.tested = ~((self.det > -DET_EPS) & (self.det < DET_EPS))
        with np.errstate(divide='ignore'):
            self.inv_det = np.where(self.tested, 1.0 / self.det, 0.0)
            self.inv_det_any = 1.0 / self.det                                  # for the ambiguity of the skip decision


def triangle_distsq(P, prep, sel=None):
    """float-rounded distsq [n, F] (inf for degenerate triangles); `sel` restricts to a triangle index array [n] -> [n]."""
    get = (lambda x: x[sel]) if sel is not None else (lambda x: x[None])
    P = P if sel is not None else P[:, None, :]
    a, b, c = get(prep.a), get(prep.b), get(prep.c)
    p0, p1, p2 = P - a, P - b, P - c
    face = np.ones(p0.shape[:-1], dtype=bool)
    for cn, pk in zip(prep.cn, (p0, p1, p2)):
        face &= ~np.signbit(_dot(get(cn), pk))
    eds = []
    for e, r, pk in zip((prep.e10, prep.e21, prep.e02), prep.r, (p0, p1, p2)):
        e = get(e)
        ck = np.clip(f32(_dot(e, pk) * get(r)), 0.0, 1.0)
        eds.append(f32(_dot(e * ck[..., None] - pk, e * ck[..., None] - pk)))
    edge = np.minimum(np.minimum(eds[0], eds[1]), eds[2])
    dn = _dot(get(prep.n), p0)
    with np.errstate(invalid='ignore', over='ignore'):
        fd = f32(dn * dn * get(prep.rn))
    d = np.where(face, fd, edge)
    d = np.where(d < 0, 0.0, d)
    return np.where(get(prep.degenerate), np.inf, d)


def stab(P, prep):
    """(pos [n,13], neg [n,13], ambiguous [n]) over all triangles."""
    P = P[:, None, None, :]                                                  # [n,1,1,3]
    tv = P - prep.a[None, :, None, :]                                        # [n,F,1,3]
    q = np.cross(tv, prep.e10[None, :, None, :])                             # [n,F,1,3]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        un = _dot(tv, prep.pvec[None])                                       # [n,F,13]
        vn = _dot(DIRS[None, None], q)
        tn = _dot(prep.e2[None, :, None, :], q)
        inv = prep.inv_det_any[None]
        u, v, t = un * inv, vn * inv, tn * inv
        hit = (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & prep.tested[None]
        pos = (hit & (t >= 0)).any(axis=1)
        neg = (hit & (t < 0)).any(axis=1)
        # ambiguity: a test whose outcome a relative 1e-9 move (or the rounding of the quantities, scaled by their conditioning)
        # could flip, for a test that could hit at all
        ntv = np.linalg.norm(tv, axis=-1)
        nq = np.linalg.norm(q, axis=-1)
        ad = np.abs(prep.det)[None]
        tol_u = AMBIGUITY + 64 * EPS64 * ntv * np.linalg.norm(prep.pvec, axis=-1)[None] / ad
        tol_v = AMBIGUITY + 64 * EPS64 * nq / ad
        tol = np.maximum(tol_u, tol_v)
        loose = (u >= -tol) & (u <= 1 + tol) & (v >= -tol) & (u + v <= 1 + tol)
        strict = (u >= tol) & (u <= 1 - tol) & (v >= tol) & (u + v <= 1 - tol)
        tol_t = AMBIGUITY * ntv + 64 * EPS64 * np.linalg.norm(prep.e2, axis=-1)[None, :, None] * nq / ad
        amb = (prep.tested[None] & loose & ~strict) | (prep.tested[None] & loose & (np.abs(t) <= tol_t))
        amb |= loose & (np.abs(ad - DET_EPS) <= AMBIGUITY * DET_EPS)
    return pos, neg, amb.any(axis=(1, 2))


def mesh_sdf(P, T, chunk_pairs=1 << 21):
    """(sdf [n] float64, nearest triangle [n] int64 (-1: all degenerate), ambiguous [n] bool, min distsq [n])."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    prep = Prepared(T)
    F = prep.a.shape[0]
    step = max(1, chunk_pairs // max(F, 1))
    sdf = np.empty(P.shape[0])
    idx = np.empty(P.shape[0], dtype=np.int64)
    amb = np.empty(P.shape[0], dtype=bool)
    mind = np.empty(P.shape[0])
    sstep = max(1, step // 13)
    for s in range(0, P.shape[0], step):
        Pc = P[s:s + step]
        d = triangle_distsq(Pc, prep)
        m = d.min(axis=1)
        mind[s:s + step] = m
        idx[s:s + step] = np.where(np.isinf(m), -1, np.argmin(d, axis=1))
        inside = np.ones(Pc.shape[0], dtype=bool)
        for k in range(0, Pc.shape[0], sstep):
            pos, neg, a = stab(Pc[k:k + sstep], prep)
            inside[k:k + sstep] = (pos & neg).all(axis=1)
            amb[s + k:s + k + sstep] = a
        mag = f32(np.sqrt(m))
        sdf[s:s + step] = np.where(inside, -mag, mag)
    return sdf, idx, amb, mind


def sdf_close(got, want):
    """|got - want| <= 2.5e-7 |want| + 1e-9 (two float ulps)."""
    got, want = np.asarray(got), np.asarray(want)
    both_inf = np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want))
    with np.errstate(invalid='ignore'):
        return both_inf | (np.abs(np.abs(got) - np.abs(want)) <= 2.5e-7 * np.abs(want) + 1e-9)


def closest_point_on_triangle(T, P):
    """Closest point of triangle k to point k by minimising over the face (barycentric projection, when inside) and the three
    edge segments - a formulation independent of the Voronoi-region method."""
    T, P = np.asarray(T, dtype=np.float64), np.asarray(P, dtype=np.float64)
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    cands = []
    for s, e in ((a, b), (b, c), (c, a)):
        d = e - s
        t = np.clip(_dot(P - s, d) / np.maximum(_dot(d, d), 1e-300), 0.0, 1.0)
        cands.append(s + t[:, None] * d)
    n = np.cross(b - a, c - a)
    nn = np.maximum(_dot(n, n), 1e-300)
    proj = P - (_dot(P - a, n) / nn)[:, None] * n
    w = [_dot(np.cross(v1 - proj, v2 - proj), n) for v1, v2 in ((b, c), (c, a), (a, b))]
    inside = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)
    cands.append(np.where(inside[:, None], proj, np.inf))
    C = np.stack(cands, 1)
    with np.errstate(invalid='ignore'):
        dist = np.linalg.norm(C - P[:, None], axis=-1)
    return C[np.arange(P.shape[0]), np.nanargmin(np.where(np.isfinite(dist), dist, np.inf), axis=1)]


# ------------------------------------------------------------------------------------------------ procedural meshes (V, F)
def box(h=0.5):
    """Axis-aligned cube [-h, h]^3, 12 triangles."""
    V = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], dtype=np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    F = [(q[0], q[1], q[2]) for q in quads] + [(q[0], q[2], q[3]) for q in quads]
    return V, np.array(F, dtype=np.int64)


def box_sdf(P, h=0.5):
    q = np.abs(P) - h
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0)


def icosphere(subdiv=2, radius=1.0):
    t = (1.0 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    V = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in V]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid = {}

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = V[i] + V[j]
                V.append(p / np.linalg.norm(p))
                mid[key] = len(V) - 1
            return mid[key]
        G = []
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    return np.array(V) * radius, np.array(F, dtype=np.int64)


def torus(R=0.6, r=0.25, nu=48, nv=24):
    """Torus around z on a wrapped (u, v) grid: non-convex, genus 1."""
    u = np.arange(nu) * 2 * np.pi / nu
    v = np.arange(nv) * 2 * np.pi / nv
    U, W = np.meshgrid(u, v, indexing='ij')
    V = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    F = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            F += [(a, b, c), (a, c, d)]
    return V, np.array(F, dtype=np.int64)


def torus_sdf(P, R=0.6, r=0.25):
    return np.hypot(np.hypot(P[:, 0], P[:, 1]) - R, P[:, 2]) - r


def bumpy_radius(D, base=0.8, amp=0.08):
    """Radius of the bumpy sphere in the unit directions D [n,3]."""
    return base * (1 + amp * np.sin(3 * D[:, 0]) * np.sin(4 * D[:, 1] + 1) * np.cos(5 * D[:, 2]))


def bumpy_sphere(subdiv=6):
    """Star-shaped: an icosphere (20 * 4^subdiv triangles: 6 -> 81920, 7 -> 327680) displaced radially by bumpy_radius."""
    V, F = icosphere(subdiv)
    return V * bumpy_radius(V)[:, None], F


def degenerate_mesh():
    """An icosphere plus duplicated triangles, zero-area triangles (a repeated vertex, three collinear vertices) and a
    needle."""
    V, F = icosphere(1, 0.7)
    nv = V.shape[0]
    extra_v = np.array([[0.1, 0.2, 0.3], [0.2, 0.4, 0.6], [0.3, 0.6, 0.9], [0.9, 0.9, 0.9]])
    V = np.concatenate([V, extra_v])
    extra_f = np.array([F[3], F[3], F[7], [nv, nv + 1, nv + 2], [nv, nv, nv + 3], [nv + 3, nv + 3, nv + 3]], dtype=np.int64)
    return V, np.concatenate([F, extra_f])


def single_triangle():
    return np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, -0.1], [0.0, 0.7, 0.2]]), np.array([[0, 1, 2]], dtype=np.int64)


def write_obj(path, V, F):
    with open(path, "w") as f:
        f.write("".join(f"v {float(x)!r} {float(y)!r} {float(z)!r}\n" for x, y, z in V))
        f.write("".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in F))
    return str(path)
