"""NumPy restatement of the device mesh decimation (``csrc/cloud_decimate.hip``):
quadric edge collapse in rounds of independent collapses.  Vectorised per round over the candidate
edges; wherever order matters (the quadric sums, the rank, the budget's prefix) the order is
written out.  The rule uses ``+ - * /`` and comparisons in fp64 and integer minima, so the device
is expected to equal these functions bit for bit.  Our rule: parity with MeshLab / VCGlib is
unpinned.  Also the meshes the decimation tests add to ``meshpost_ref``'s builders.
"""
import functools

import numpy as np

import meshpost_ref as P

SWEEPS = 4
REASONS = ("boundary", "nonmanifold", "link", "valence", "flip", "nan")        # the record's order
STATS = REASONS + ("valid", "selected")
_ORDER = ("boundary", "nonmanifold", "link", "valence", "nan", "flip")          # the order of the tests


# ------------------------------------------------------------------ the named expressions
def cross(A, B, C):
    """``n = e1 x e2`` of corners in winding order, not normalised; rows of ``[.., 3]``."""
    e1, e2 = B - A, C - A
    return np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                     e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], axis=-1)


def triangle_quadrics(V, T):
    """``K = (a2, ab, ac, ad, b2, bc, bd, c2, cd, d2)`` per triangle, float64 ``[T, 10]``."""
    A = V[T[:, 0]]
    n = cross(A, V[T[:, 1]], V[T[:, 2]])
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    d = -((nx * A[:, 0] + ny * A[:, 1]) + nz * A[:, 2])
    return np.stack([nx * nx, nx * ny, nx * nz, nx * d, ny * ny, ny * nz, ny * d, nz * nz, nz * d, d * d], axis=1)


def incidence(T, nv):
    """``(offsets int64 [nv + 1], triangles)``: per vertex its corners' triangles, ascending."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    vert, tri = T.ravel(), np.repeat(np.arange(len(T)), 3)
    order = np.lexsort((tri, vert))
    return np.concatenate([[0], np.cumsum(np.bincount(vert, minlength=nv))]).astype(np.int64), tri[order]


def vertex_quadrics(V, T):
    """``Q[v] = ((K0 + K1) + K2) + ..`` over the incident triangles in ascending index."""
    K = triangle_quadrics(V, np.asarray(T, np.int64))
    off, tri = incidence(T, len(V))
    cnt = np.diff(off)
    Q = np.zeros((len(V), 10))
    have = np.flatnonzero(cnt > 0)
    Q[have] = K[tri[off[have]]]
    for k in range(1, int(cnt.max(initial=0))):
        sel = np.flatnonzero(cnt > k)
        Q[sel] = Q[sel] + K[tri[off[sel] + k]]
    return Q


def cost_at(q, p):
    """The quadric's value at ``p``; a non-finite cost counts as +inf, anything not above 0 as 0.0."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r0 = ((q[:, 0] * x + q[:, 1] * y) + q[:, 2] * z) + q[:, 3]
    r1 = ((q[:, 1] * x + q[:, 4] * y) + q[:, 5] * z) + q[:, 6]
    r2 = ((q[:, 2] * x + q[:, 5] * y) + q[:, 7] * z) + q[:, 8]
    r3 = ((q[:, 3] * x + q[:, 6] * y) + q[:, 8] * z) + q[:, 9]
    c = ((r0 * x + r1 * y) + r2 * z) + r3
    return np.where(np.isfinite(c), np.where(c > 0.0, c, 0.0), np.inf)


def d2(d):
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def placement(Pv, Q, u, v, bu, bv):
    """``(p [n, 3], cost [n])`` of the candidates ``(u, v)``; the cost is +inf where it is not finite."""
    q = Q[u] + Q[v]
    pu, pv = Pv[u], Pv[v]
    mid = (pu + pv) * 0.5
    c00, c01, c02 = q[:, 4] * q[:, 7] - q[:, 5] * q[:, 5], q[:, 2] * q[:, 5] - q[:, 1] * q[:, 7], q[:, 1] * q[:, 5] - q[:, 2] * q[:, 4]
    c11, c12, c22 = q[:, 0] * q[:, 7] - q[:, 2] * q[:, 2], q[:, 1] * q[:, 2] - q[:, 0] * q[:, 5], q[:, 0] * q[:, 4] - q[:, 1] * q[:, 1]
    det = (q[:, 0] * c00 + q[:, 1] * c01) + q[:, 2] * c02
    r0, r1, r2 = -q[:, 3], -q[:, 6], -q[:, 8]
    s = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                  ((c02 * r0 + c12 * r1) + c22 * r2) / det], axis=1)
    admitted = (det != 0.0) & np.isfinite(s).all(axis=1) & (d2(s - mid) <= 4.0 * d2(pv - pu))
    cands = np.stack([s, pu, pv, mid])                                      # the order of the choice
    costs = np.stack([cost_at(q, c) for c in cands])
    costs[0, ~admitted] = np.inf
    # the smallest wins, ties to the earliest; where s is not admitted and all are +inf, P[u]
    pick = np.where(admitted | (costs[1:].min(axis=0) < np.inf), np.argmin(costs, axis=0), 1)
    pick = np.where(bu, 1, np.where(bv, 2, pick))
    idx = np.arange(len(u))
    return cands[pick, idx], costs[pick, idx]


def _flips(Pv, T, ioff, itri, w, other, p):
    """Whether a triangle at ``w`` without ``other`` turns over (or degenerates) when ``w`` moves to ``p``."""
    flip = np.zeros(len(w), bool)
    cnt = ioff[w + 1] - ioff[w]
    for k in range(int(cnt.max(initial=0))):
        sel = np.flatnonzero(cnt > k)
        tri = T[itri[ioff[w[sel]] + k]]
        sel, tri = sel[~(tri == other[sel, None]).any(axis=1)], tri[~(tri == other[sel, None]).any(axis=1)]
        before = Pv[tri]                                                    # [m, 3 corners, 3]
        after = np.where((tri == w[sel, None])[:, :, None], p[sel, None, :], before)
        n0, n1 = cross(before[:, 0], before[:, 1], before[:, 2]), cross(after[:, 0], after[:, 1], after[:, 2])
        dot = (n0[:, 0] * n1[:, 0] + n0[:, 1] * n1[:, 1]) + n0[:, 2] * n1[:, 2]
        flip[sel[~(dot > 0.0)]] = True
    return flip


def _closed(off, nbr, u, v):
    """The closed neighbourhoods ``N(u) u N(v) u {u, v}`` flattened: ``(candidate, vertex)`` pairs.
    The edge exists, so ``u`` is in ``N(v)`` and ``v`` in ``N(u)``: the two rows are all of it."""
    cid, vert = [], []
    for w in (u, v):
        cnt = off[w + 1] - off[w]
        c = np.repeat(np.arange(len(w)), cnt)
        cid.append(c)
        vert.append(nbr[off[w][c] + (np.arange(len(c)) - np.repeat(np.cumsum(cnt) - cnt, cnt))])
    return np.concatenate(cid), np.concatenate(vert).astype(np.int64)


# ------------------------------------------------------------------ a round
def one_round(Pv, Q, T, target):
    """One round on the alive triangles ``T``: ``(Pv, Q, T, dead vertices, stats dict, applied)``;
    ``Pv`` and ``Q`` are updated in place."""
    nv = len(Pv)
    T = np.asarray(T, np.int64).reshape(-1, 3)
    adj = P.adjacency(T, nv)
    off, nbr, bnd = adj["offsets"], adj["neighbours"].astype(np.int64), adj["boundary"].astype(bool)
    deg = np.diff(off)
    D = P.winding_pairs(T)
    dkey = (D[:, 0] << 32) | D[:, 1]                                        # ascending
    src = np.repeat(np.arange(nv), deg)
    nkey = (src << 32) | nbr
    m = src < nbr
    u, v = src[m], nbr[m]                                                   # the candidates, ascending key
    n = len(u)
    fail = {}
    fail["boundary"] = bnd[u] & bnd[v]
    once = np.ones(n, bool)
    for k in ((u << 32) | v, (v << 32) | u):
        once &= (np.searchsorted(dkey, k, "right") - np.searchsorted(dkey, k, "left")) == 1
    fail["nonmanifold"] = ~once
    common, thin = np.zeros(n, np.int64), np.zeros(n, bool)
    for k in range(int(deg[u].max(initial=0))):                             # the k-th neighbour of u: is it one of v's?
        sel = np.flatnonzero(deg[u] > k)
        w = nbr[off[u[sel]] + k]
        key = (v[sel] << 32) | w
        at = np.searchsorted(nkey, key)
        hit = (at < len(nkey)) & (nkey[np.minimum(at, len(nkey) - 1)] == key)
        common[sel] += hit
        thin[sel] |= hit & (deg[w] < 4)
    fail["link"] = common != 2
    fail["valence"] = thin
    ioff, itri = incidence(T, nv)
    with np.errstate(all="ignore"):
        p, cost = placement(Pv, Q, u, v, bnd[u], bnd[v])
        fail["nan"] = ~(cost < np.inf)
        fail["flip"] = _flips(Pv, T, ioff, itri, u, v, p) | _flips(Pv, T, ioff, itri, v, u, p)
    reason = np.full(n, -1)
    for name in reversed(_ORDER):                                           # the first test failed names the refusal
        reason[fail[name]] = REASONS.index(name)
    valid = reason < 0
    stats = {name: int((reason == i).sum()) for i, name in enumerate(REASONS)}
    stats["valid"] = int(valid.sum())
    # rank by (cost bits, key): a stable sort of the key-ordered valid candidates by cost
    vi = np.flatnonzero(valid)
    order = vi[np.argsort(np.ascontiguousarray(cost[vi]).view(np.uint64), kind="stable")]
    rank = np.full(n, np.iinfo(np.int64).max)
    rank[order] = np.arange(len(order))
    cid, vert = _closed(off, nbr, u, v)
    claimed, selected = np.zeros(nv, bool), np.zeros(n, bool)
    for _ in range(SWEEPS):
        live = valid & ~selected & (np.bincount(cid, weights=claimed[vert], minlength=n) == 0)
        lm = live[cid]
        word = np.full(nv, np.iinfo(np.int64).max)
        np.minimum.at(word, vert[lm], rank[cid[lm]])
        lost = np.bincount(cid[lm], weights=word[vert[lm]] != rank[cid[lm]], minlength=n) > 0
        pick = live & ~lost
        selected |= pick
        claimed[vert[pick[cid]]] = True
    stats["selected"] = int(selected.sum())
    need = (len(T) - target + 1) // 2
    apply = order[selected[order]][:need]                                   # the budget's prefix in rank order
    ua, va = u[apply], v[apply]
    Pv[ua] = p[apply]
    Q[ua] = Q[ua] + Q[va]
    remap = np.arange(nv)
    remap[va] = ua
    T = remap[T]
    T = T[(T[:, 0] != T[:, 1]) & (T[:, 1] != T[:, 2]) & (T[:, 2] != T[:, 0])]
    return T, va, stats, len(apply)


def decimate(V, T, target, max_rounds=512, D=None):
    """``mesh.decimate_quadric``: ``(vertices, triangles int32, densities or None, record)``."""
    V = np.array(V, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.int64).reshape(-1, 3)
    if len(T) and not (0 <= T.min() and T.max() < len(V)):
        raise IndexError("a triangle index lies outside 0 .. V - 1")
    rec = dict(faces_in=len(T), faces_out=len(T), rounds=0, collapses=0, stop="target", **{k: 0 for k in STATS})
    dead = np.zeros(len(V), bool)
    if len(V) and len(T):
        with np.errstate(all="ignore"):
            Q = vertex_quadrics(V, T)
        while True:
            if len(T) <= target:
                rec["stop"] = "target"
                break
            if rec["rounds"] >= max_rounds:
                rec["stop"] = "max_rounds"
                break
            T, gone, stats, applied = one_round(V, Q, T, target)
            dead[gone] = True
            rec["rounds"] += 1
            rec["collapses"] += applied
            rec.update(stats)
            if applied == 0:
                rec["stop"] = "no_valid_edge"
                break
    rec["faces_out"] = len(T)
    new_id = np.cumsum(~dead) - 1
    return V[~dead], new_id[T].astype(np.int32).reshape(-1, 3), None if D is None else np.asarray(D, np.float64)[~dead], rec


def euler(T):
    """V - E + F over the referenced vertices."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]]), axis=1)
    return len(np.unique(T)) - len(np.unique(e, axis=0)) + len(T)


# ------------------------------------------------------------------ mesh builders
def bipyramid(n=80):
    """An n-gon with an apex on each side (vertices 0 and 1, the ring 2 .. n + 1): closed, the two
    apex rows are longer than a wavefront, and every ring edge has both apexes as its common
    neighbours.  The ring is wavy, so the costs differ."""
    ang = 2.0 * np.pi * np.arange(n) / n
    r = 1.0 + 0.1 * np.cos(5 * ang)
    ring = np.stack([r * np.cos(ang), r * np.sin(ang), 0.05 * np.sin(3 * ang)], axis=1)
    V = np.concatenate([[[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], ring])
    T = []
    for i in range(n):
        a, b = 2 + i, 2 + (i + 1) % n
        T += [[0, a, b], [1, b, a]]
    return P._mesh(V, T)


def planar_patch(nx=8, ny=8):
    """``grid_patch`` with ``z = 0``: every cost is exactly 0 and every ``det`` is 0, so the rank is
    the key alone and the placement falls to ``P[u]`` by the tie rule."""
    return P.grid_patch(nx, ny)


def nan_vertex_patch():
    """A bumpy 6 x 6 patch whose interior vertex 24 is NaN: every edge at it is refused (its cost
    is not finite) and so is every edge whose flip test reads it; the rest proceeds."""
    V, T = P.grid_patch(6, 6, seed=7)
    V = V.copy()
    V[24] = np.nan
    return V, T


BUILDERS = {**P.BUILDERS, "bipyramid": bipyramid, "planar": planar_patch, "lattice": P.punched_lattice,
            "nan_vertex": nan_vertex_patch,
            # bumpy open patches around one 256-thread block: 255, 256 and 258 triangles, 249 and 261
            # candidate edges; 1,152 triangles and 1,776 edges over several blocks
            "patch8x16cut": lambda: (lambda V, T: (V, T[:255].copy()))(*P.grid_patch(8, 16, seed=4)),
            "patch8x16": lambda: P.grid_patch(8, 16, seed=4), "patch3x43": lambda: P.grid_patch(3, 43, seed=2),
            "patch7x11": lambda: P.grid_patch(7, 11, seed=1), "patch9x9": lambda: P.grid_patch(9, 9, seed=5),
            "patch24x24": lambda: P.grid_patch(24, 24, seed=3)}


@functools.lru_cache(maxsize=None)
def built(name):
    """``(V, T, D)`` of a builder, read-only; the densities are made up (one per vertex, all different)."""
    V, T = BUILDERS[name]()
    V, T = np.ascontiguousarray(V, np.float64), np.ascontiguousarray(T, np.int32)
    D = 0.5 * np.arange(len(V), dtype=np.float64) + 1.0
    for a in (V, T, D):
        a.setflags(write=False)
    return V, T, D


@functools.lru_cache(maxsize=None)
def reference(name, target, max_rounds=512):
    """``decimate`` of a builder, computed once and shared read-only."""
    V, T, D = built(name)
    Vo, To, Do, rec = decimate(V, T, target, max_rounds, D)
    for a in (Vo, To, Do):
        a.setflags(write=False)
    return Vo, To, Do, rec
