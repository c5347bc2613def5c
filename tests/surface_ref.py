"""NumPy restatement of the device surface mesher (csrc/cloud_surface.hip):
the empty-ball triangles of an oriented cloud, radius by radius.  Test infrastructure.

Ball pivoting as Open3D runs it is a sequential front; what it converges to is not.  Its triangles
are those on which a ball of radius ``r`` rests, on the normals' side, with no point inside.  That
set is a pure function of the cloud; where two such triangles would use one directed edge, a total
order (the circumradius' bits, then the indices) decides.  Our rule, Open3D parity unpinned.

Every expression is written in the order the device evaluates it (float64, no contraction), so the
device equals this bit for bit.  The functions named ``*_rule`` are the expressions themselves.

The rule, for radii ``r_1 < .. < r_K`` and the state ``taken`` (directed edges) and ``closed``
(vertices), both empty at the start; in pass ``k`` with ``r = r_k``:

* candidates: every triple ``a < b < c`` of vertices that are not closed whose three squared side
  lengths are ``< 4 r^2`` and that passes :func:`triple_rule` (not flat, circumradius at most ``r``,
  the three normals on one side of its plane, no other point inside the ball resting on it);
* rank: ascending ``(bits of rho^2, a, b, c)``;
* selection: greedy in rank order, a candidate is accepted iff none of its three directed edges (in
  its winding) is taken; :func:`select_rounds` is the same set, found the way the device finds it;
* afterwards ``closed[v]`` iff ``v`` has a taken edge and every taken edge at ``v`` has its reverse.

An anchor ``a`` with more than :data:`CAP` open neighbours of higher index within ``2 r`` is
refused (``ValueError``): the device stages that list in LDS.
"""
import numpy as np
from scipy.spatial import cKDTree

CAP = 512                        # kMaxPartners of csrc/cloud_surface.hip
MAX_RADII = 8
SLACK = 1.0 - 2.0 ** -30         # a fourth cospherical point stays outside the ball


# ----------------------------------------------------------------------------- the expressions
def dot_rule(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def d2_rule(d):
    """``d2_rule`` of csrc/cloud_grid.h."""
    return dot_rule(d, d)


def cross_rule(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1],
                     x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def triple_rule(pa, pb, pc, na, nb, nc, r2):
    """The geometry of triples ``a < b < c`` (arrays ``[m, 3]``): ``(ok, sign, rho2, o)``.  ``ok``:
    the triple is not flat, its circumradius is at most ``r`` and its three normals agree; ``sign``
    +1 for the triangle ``(a, b, c)``, -1 for ``(a, c, b)``; ``o`` the centre of the ball."""
    with np.errstate(all="ignore"):
        u, v = pb - pa, pc - pa
        w = cross_rule(u, v)
        w2 = dot_rule(w, w)
        ok = w2 > 0.0
        uu, vv = dot_rule(u, u), dot_rule(v, v)
        cc = (cross_rule(w, u) * vv[:, None] + cross_rule(v, w) * uu[:, None]) / (2.0 * w2)[:, None]
        rho2 = dot_rule(cc, cc)
        h2 = r2 - rho2
        ok &= h2 >= 0.0
        sa, sb, sc = dot_rule(w, na), dot_rule(w, nb), dot_rule(w, nc)
        pos = (sa > 0.0) & (sb > 0.0) & (sc > 0.0)
        neg = (sa < 0.0) & (sb < 0.0) & (sc < 0.0)
        ok &= pos | neg
        t = np.sqrt(h2 / w2)
        t = np.where(neg, -t, t)
        o = (pa + cc) + t[:, None] * w
    return ok, np.where(neg, -1, 1), rho2, o


def edge_keys(tri):
    """The three directed edges of triangles ``[m, 3]`` in their winding, as ``src << 32 | dst``: ``[m, 3]`` uint64."""
    t = np.asarray(tri).astype(np.uint64).reshape(-1, 3)
    return (t << np.uint64(32)) | t[:, [1, 2, 0]]


# ----------------------------------------------------------------------------- a pass
def candidates(P, Nrm, r, closed, tree=None):
    """The candidates of one pass in rank order: ``(tri int32 [C, 3] in winding, rho_bits uint64 [C])``."""
    P, Nrm = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(Nrm, np.float64)
    n = len(P)
    tree = tree if tree is not None else cKDTree(P)
    r2 = r * r
    r2x4, r2s = 4.0 * r2, r2 * SLACK
    near = tree.query_ball_point(P, 2.0 * r * (1.0 + 1e-9))        # supersets: the rules below decide
    block = tree.query_ball_point(P, 3.0 * r)
    tris, rhos, abcs = [], [], []
    for a in range(n):
        if closed[a]:
            continue
        nb = np.array(sorted(near[a]), np.int64)
        nb = nb[(nb > a) & ~closed[nb]]
        nb = nb[d2_rule(P[nb] - P[a]) < r2x4]
        if len(nb) > CAP:
            raise ValueError(f"radius {r!r}: a point has more than {CAP} open neighbours of higher index within 2 r")
        if len(nb) < 2:
            continue
        i, j = np.triu_indices(len(nb), 1)
        b, c = nb[i], nb[j]
        keep = d2_rule(P[c] - P[b]) < r2x4
        b, c = b[keep], c[keep]
        pa = np.broadcast_to(P[a], (len(b), 3))
        na = np.broadcast_to(Nrm[a], (len(b), 3))
        ok, sign, rho2, o = triple_rule(pa, P[b], P[c], na, Nrm[b], Nrm[c], r2)
        b, c, sign, rho2, o = b[ok], c[ok], sign[ok], rho2[ok], o[ok]
        if not len(b):
            continue
        blk = np.array(block[a], np.int64)
        with np.errstate(all="ignore"):
            inside = d2_rule(P[blk][None, :, :] - o[:, None, :]) < r2s
        inside &= ~((blk[None, :] == a) | (blk[None, :] == b[:, None]) | (blk[None, :] == c[:, None]))
        empty = ~inside.any(axis=1)
        b, c, sign, rho2 = b[empty], c[empty], sign[empty], rho2[empty]
        av = np.full(len(b), a, np.int64)
        tris.append(np.where(sign[:, None] > 0, np.stack([av, b, c], 1), np.stack([av, c, b], 1)))
        abcs.append(np.stack([av, b, c], 1))
        rhos.append(rho2.view(np.uint64))
    if not tris:
        return np.zeros((0, 3), np.int32), np.zeros(0, np.uint64)
    tri, abc, rho = np.concatenate(tris), np.concatenate(abcs), np.concatenate(rhos)
    order = np.lexsort((abc[:, 2], abc[:, 1], abc[:, 0], rho))
    return tri[order].astype(np.int32), rho[order]


def select_greedy(tri, taken):
    """Greedy in rank order against the set ``taken`` (not changed): the accepted flags ``[C]``."""
    taken = set(taken)
    acc = np.zeros(len(tri), bool)
    for r, keys in enumerate(edge_keys(tri).tolist()):
        if not (keys[0] in taken or keys[1] in taken or keys[2] in taken):
            acc[r] = True
            taken.update(keys)
    return acc


def select_rounds(tri, taken, max_rounds=64):
    """The same selection in rounds: ``(accepted flags, rounds)``.  A round: every live candidate
    offers its rank to its three edges, those that hold the minimum on all three are accepted,
    and the live candidates on an edge accepted now are dropped; live at the start are those
    without an edge of an earlier pass.  No candidates: no round."""
    C = len(tri)
    acc = np.zeros(C, bool)
    if C == 0:
        return acc, 0
    keys = edge_keys(tri)
    uniq, slot = np.unique(keys.reshape(-1), return_inverse=True)
    slot = slot.reshape(C, 3)
    marked = np.isin(uniq, np.fromiter(taken, np.uint64, len(taken)))
    live = ~marked[slot].any(axis=1)
    rank = np.arange(C, dtype=np.int64)
    rounds = 0
    while True:
        if rounds >= max_rounds:
            raise RuntimeError(f"the selection did not end in {max_rounds} rounds")
        rounds += 1
        word = np.full(len(uniq), C, np.int64)
        np.minimum.at(word, slot[live].reshape(-1), np.repeat(rank[live], 3))
        win = live & (word[slot] == rank[:, None]).all(axis=1)
        acc |= win
        marked[slot[win].reshape(-1)] = True
        live &= ~marked[slot].any(axis=1)
        if not live.any():
            return acc, rounds


def closed_rule(taken, n):
    """``closed[v]``: ``v`` has a taken edge and every taken edge at ``v`` has its reverse."""
    has, opened = np.zeros(n, bool), np.zeros(n, bool)
    for k in taken:
        s, d = k >> 32, k & 0xFFFFFFFF
        has[s] = has[d] = True
        if ((d << 32) | s) not in taken:
            opened[s] = opened[d] = True
    return has & ~opened


def check_radii(radii):
    rs = [float(x) for x in np.asarray(radii, np.float64).reshape(-1)]
    if not 1 <= len(rs) <= MAX_RADII:
        raise ValueError("radii: between 1 and 8")
    if not all(np.isfinite(x) and x > 0.0 for x in rs) or any(b <= a for a, b in zip(rs, rs[1:])):
        raise ValueError("radii: finite, positive, strictly ascending")
    return rs


def ball_pivot(P, Nrm, radii, form="greedy", max_rounds=64):
    """``(triangles int32 [T, 3], record, closed)``: the passes in order, within a pass ascending
    rank; ``record`` one dict per pass (``radius``, ``candidates``, ``accepted``, ``rounds``).
    ``form="rounds"`` selects by :func:`select_rounds` instead of the greedy; the rounds are
    counted either way."""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    if not np.isfinite(P).all():
        raise ValueError("the cloud holds a NaN or infinite coordinate")
    tree = cKDTree(P) if n else None
    taken, closed = set(), np.zeros(n, bool)
    out, record = [], []
    for r in check_radii(radii):
        if n < 3:
            record.append(dict(radius=r, candidates=0, accepted=0, rounds=0))
            continue
        tri, _ = candidates(P, Nrm, r, closed, tree)
        acc_r, rounds = select_rounds(tri, taken, max_rounds)
        acc = acc_r if form == "rounds" else select_greedy(tri, taken)
        kept = tri[acc]
        out.append(kept)
        taken.update(edge_keys(kept).reshape(-1).tolist())
        closed = closed_rule(taken, n)
        record.append(dict(radius=r, candidates=len(tri), accepted=len(kept), rounds=rounds))
    tris = np.concatenate(out) if out else np.zeros((0, 3), np.int32)
    return tris.astype(np.int32).reshape(-1, 3), record, closed


# ----------------------------------------------------------------------------- what the tests look at
def directed_edges(tri):
    return edge_keys(tri).reshape(-1)


def topology(tri, n_vertices):
    """``(no directed edge twice, boundary edges, Euler characteristic over the referenced vertices)``."""
    k = directed_edges(tri)
    once = len(np.unique(k)) == len(k)
    rev = ((k & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | (k >> np.uint64(32))
    boundary = int((~np.isin(rev, k)).sum())
    und = np.unique(np.minimum(k, rev))
    V = len(np.unique(np.asarray(tri).reshape(-1)))
    return once, boundary, V - len(und) + len(tri)


def agrees_with_normals(P, Nrm, tri):
    a, b, c = (np.asarray(tri)[:, i] for i in range(3))
    w = cross_rule(P[b] - P[a], P[c] - P[a])
    return bool(((dot_rule(w, Nrm[a]) > 0) & (dot_rule(w, Nrm[b]) > 0) & (dot_rule(w, Nrm[c]) > 0)).all())


# ----------------------------------------------------------------------------- the clouds
def mean_nn(P):
    return float(np.mean(cKDTree(P).query(P, 2)[0][:, 1]))


def fibonacci_sphere(n, noise=0.0, seed=0):
    """``(P, Nrm)``: ``n`` points of the golden-angle spiral on the unit sphere, outward normals;
    ``noise``: a relative radial and an absolute positional disturbance of that size."""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    Nrm = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)
    P = Nrm.copy()
    if noise:
        rng = np.random.default_rng(seed)
        P = P * (1.0 + noise * rng.uniform(-1, 1, (n, 1))) + noise * mean_nn(P) * rng.uniform(-1, 1, (n, 3))
    return np.ascontiguousarray(P), np.ascontiguousarray(Nrm)


def lattice(nx, ny, jitter=0.0, seed=0, hole=None, z_jitter=0.0):
    """``(P, Nrm)``: the unit lattice ``nx x ny`` in the plane z = 0 with normals +z; ``jitter``
    moves x and y by up to that much, ``hole = (x0, y0, w)`` leaves out a ``w x w`` block."""
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    keep = np.ones(x.shape, bool)
    if hole is not None:
        x0, y0, w = hole
        keep[x0:x0 + w, y0:y0 + w] = False
    P = np.stack([x[keep], y[keep], np.zeros(int(keep.sum()))], 1)
    rng = np.random.default_rng(seed)
    if jitter:
        P[:, :2] += rng.uniform(-jitter, jitter, (len(P), 2))
    if z_jitter:
        P[:, 2] += rng.uniform(-z_jitter, z_jitter, len(P))
    Nrm = np.zeros_like(P)
    Nrm[:, 2] = 1.0
    return np.ascontiguousarray(P), Nrm


def shuffled(P, Nrm, seed=0):
    perm = np.random.default_rng(seed).permutation(len(P))
    return np.ascontiguousarray(P[perm]), np.ascontiguousarray(Nrm[perm])


def hub(n_partners):
    """``(P, Nrm)``: point 0 with ``n_partners`` points on the circle of radius 1.9 around it in
    the plane z = 0, so at ``r = 1`` every one of them is an open neighbour of higher index within
    ``2 r`` of point 0.  Three points of the circle have a circumradius of 1.9 and fail at once; the
    circle's normals are radial, which refuses the triples through point 0 (normal +z), but for
    two in every eight, whose normals are +z too: those go on to the walk for a point inside, and
    the neighbours among them have an empty ball."""
    phi = 2.0 * np.pi * np.arange(n_partners) / n_partners
    ring = np.stack([np.cos(phi), np.sin(phi), np.zeros(n_partners)], 1)
    Nrm = np.concatenate([[[0.0, 0.0, 1.0]], ring])
    Nrm[1::8] = Nrm[2::8] = [0.0, 0.0, 1.0]
    P = np.concatenate([np.zeros((1, 3)), 1.9 * ring])
    return np.ascontiguousarray(P), np.ascontiguousarray(Nrm)


# The GPU tests' clouds (tests/test_gpu_surface.py, tests/test_gpu_surface_stale.py): the smallest
# at which each part of the device code can go wrong.  2,500 points span two 2,048-point reduction
# chunks, three 1,024-point LDS tiles and ten 256-lane blocks; they are shuffled, so the grid's
# sorted order is not the input's.  One radius near 1.5 spacings there keeps the restatement quick.
def _case(name):
    if name == "three":
        return np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.tile([0.0, 0, 1], (3, 1)), [1.0]
    if name == "square":
        return (*lattice(2, 2), [1.0])
    if name == "duplicate":
        P, Nrm = lattice(5, 5, 0.1, seed=4)
        return np.concatenate([P, P[12:13]]), np.concatenate([Nrm, Nrm[12:13]]), [1.0, 2.0]
    if name == "n130":
        P, Nrm = shuffled(*fibonacci_sphere(130, 0.01, seed=6), seed=7)
        return P, Nrm, [mean_nn(P), 2.0 * mean_nn(P)]
    if name == "n1":
        return np.array([[1.0, 2.0, 3.0]]), np.array([[0.0, 0, 1]]), [1.0, 2.0]
    if name == "sphere2500":
        P, Nrm = shuffled(*fibonacci_sphere(2500, 0.01, seed=8), seed=9)
        return P, Nrm, [1.5 * mean_nn(P)]
    if name == "plane2500":
        P, Nrm = shuffled(*lattice(50, 50, 0.2, seed=10, z_jitter=0.05), seed=11)
        return P, Nrm, [1.5]
    if name == "holed":
        return (*lattice(14, 14, 0.15, seed=3, hole=(5, 5, 4)), [1.0, 2.0, 4.0])
    if name == "holed_exact":
        return (*lattice(14, 14, hole=(5, 5, 4)), [1.0, 2.0, 4.0])
    if name == "outlier":
        P, Nrm = lattice(9, 9, 0.2, seed=12)
        return np.concatenate([P, [[5e4, -3e4, 7e4]]]), np.concatenate([Nrm, [[0.0, 0, 1]]]), [1.0, 2.0]
    if name == "at_cap":
        return (*hub(CAP), [1.0])
    if name == "over_cap":
        return (*hub(CAP + 1), [1.0])
    raise KeyError(name)


_CASES = {}


def case(name):
    """``(P, Nrm, radii)`` of a named cloud, built once."""
    if name not in _CASES:
        P, Nrm, radii = _case(name)
        P, Nrm = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(Nrm, np.float64)
        P.setflags(write=False)
        Nrm.setflags(write=False)
        _CASES[name] = (P, Nrm, radii)
    return _CASES[name]


_REFERENCES = {}


def reference(name):
    """``ball_pivot`` of a named cloud, computed once and shared."""
    if name not in _REFERENCES:
        T, rec, closed = ball_pivot(*case(name))
        T.setflags(write=False)
        _REFERENCES[name] = (T, rec, closed)
    return _REFERENCES[name]
