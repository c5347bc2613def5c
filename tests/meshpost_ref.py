"""NumPy restatement of the device mesh post-processing (``csrc/cloud_meshpost.hip``, DESIGN.md
§17): vertex adjacency and boundary CSRs, Laplacian and Taubin smoothing, hole closing by ear
clipping.  Plain loops wherever order matters; the rules use ``+ - * /`` and comparisons in fp64, so
the device is expected to equal these functions bit for bit.  Our rules: parity with MeshLab /
VCGlib is unpinned.  Also the small meshes the tests are built from.
"""
import functools

import numpy as np

import mesh_ref as MR

MAX_SIZE = 64


# ------------------------------------------------------------------ connectivity
def winding_pairs(T):
    """The directed pairs a->b, b->c, c->a of every triangle, as sorted ``(src, dst)`` rows with
    their duplicates."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    d = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    return d[np.lexsort((d[:, 1], d[:, 0]))]


def _csr(pairs, nv):
    """Unique pairs without self-pairs -> ``(offsets int64 [nv + 1], neighbours int32)``."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    pairs = np.unique(pairs, axis=0)                    # ascending (src, dst)
    offsets = np.zeros(nv + 1, np.int64)
    np.add.at(offsets, pairs[:, 0] + 1, 1)
    return np.cumsum(offsets), pairs[:, 1].astype(np.int32)


def boundary_edges(T):
    """B: the winding pairs ``(a, b)`` whose reverse ``(b, a)`` is no winding pair, unique, in
    ascending key order, int64 ``[nB, 2]``."""
    d = winding_pairs(T)
    have = {(int(a), int(b)) for a, b in d}
    out = sorted({(int(a), int(b)) for a, b in d if (int(b), int(a)) not in have})
    return np.array(out, np.int64).reshape(-1, 2)


def adjacency(T, nv):
    """``dict(offsets, neighbours, boundary, boundary_offsets, boundary_neighbours)``."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    six = np.concatenate([T[:, [0, 1]], T[:, [1, 0]], T[:, [1, 2]], T[:, [2, 1]], T[:, [2, 0]], T[:, [0, 2]]])
    off, nbr = _csr(six, nv)
    B = boundary_edges(T)
    boff, bnbr = _csr(np.concatenate([B, B[:, ::-1]]), nv)
    return dict(offsets=off, neighbours=nbr, boundary=(np.diff(boff) > 0).astype(np.uint8), boundary_offsets=boff,
                boundary_neighbours=bnbr)


# ------------------------------------------------------------------ smoothing
def smooth_pass(P, adj, mode, factor=0.0):
    """One Jacobi pass.  ``mode`` "laplacian": ``p' = (p + s) / (c + 1)``; "step": ``m = s / c``,
    ``p' = p + (m - p) * factor``.  ``s = ((q0 + q1) + q2) + ..`` in row order."""
    out = P.copy()
    if len(adj["neighbours"]) == 0:
        return out
    b = adj["boundary"].astype(bool)
    lo = np.where(b, adj["boundary_offsets"][:-1], adj["offsets"][:-1])
    cnt = np.where(b, np.diff(adj["boundary_offsets"]), np.diff(adj["offsets"]))
    # one list for both kinds of row, the boundary rows behind the adjacency rows
    rows = np.concatenate([adj["neighbours"], adj["boundary_neighbours"]]).astype(np.int64)
    lo = lo + np.where(b, len(adj["neighbours"]), 0)
    live = np.flatnonzero(cnt > 0)
    s = np.zeros_like(P)
    s[live] = P[rows[lo[live]]]
    for k in range(1, int(cnt.max())):                 # the k-th neighbour of every row that has one: s = s + q_k
        sel = np.flatnonzero(cnt > k)
        s[sel] = s[sel] + P[rows[lo[sel] + k]]
    c = cnt[live].astype(np.float64)[:, None]
    if mode == "laplacian":
        out[live] = (P[live] + s[live]) / (c + 1.0)
    else:
        m = s[live] / c
        out[live] = P[live] + (m - P[live]) * np.float64(factor)
    return out


def smooth_laplacian(V, T, iterations):
    adj = adjacency(T, len(V))
    P = np.array(V, np.float64)
    for _ in range(iterations):
        P = smooth_pass(P, adj, "laplacian")
    return P


def smooth_taubin(V, T, iterations, lam=0.5, mu=-0.53):
    adj = adjacency(T, len(V))
    P = np.array(V, np.float64)
    for _ in range(iterations):
        P = smooth_pass(smooth_pass(P, adj, "step", lam), adj, "step", mu)
    return P


# ------------------------------------------------------------------ holes
def boundary_loops(T, nv, max_size=30):
    """``(record, loops)``: the counts of ``mesh.boundary_loops`` and the closable loops as
    ``(leader index in B, ring of vertex ids from the leader's source in walk order)``."""
    assert 3 <= max_size <= MAX_SIZE
    d = winding_pairs(T)
    B = boundary_edges(T)
    nb = len(B)
    blocked = np.zeros(nv, bool)
    for i in range(1, len(d)):
        if d[i, 0] == d[i - 1, 0] and d[i, 1] == d[i - 1, 1]:
            blocked[d[i, 0]] = blocked[d[i, 1]] = True
    outdeg, indeg = np.bincount(B[:, 0], minlength=nv), np.bincount(B[:, 1], minlength=nv)
    blocked |= ((outdeg + indeg) > 0) & ((outdeg != 1) | (indeg != 1))
    first = {}
    for j in range(nb - 1, -1, -1):
        first[int(B[j, 0])] = j
    nxt = [first.get(int(B[j, 1]), -1) for j in range(nb)]
    rec = dict(boundary_edges=nb, closable_loops=0, closable_edges=0, open_by_size_edges=0, blocked_edges=0, new_triangles=0)
    loops = []
    for j in range(nb):
        e, least, state, ring = j, j, "long", []
        for step in range(1, max_size + 1):
            if blocked[B[e, 0]] or blocked[B[e, 1]]:
                state = "blocked"
                break
            ring.append(int(B[e, 0]))
            e = nxt[e]
            if e < 0:
                state = "blocked"
                break
            if e == j:
                state = "closable" if step >= 3 else "blocked"
                break
            least = min(least, e)
        if state == "closable":
            rec["closable_edges"] += 1
            if least == j:
                rec["closable_loops"] += 1
                rec["new_triangles"] += len(ring) - 2
                loops.append((j, ring))
        elif state == "long":
            rec["open_by_size_edges"] += 1
        else:
            rec["blocked_edges"] += 1
    return rec, loops


def clip_ring(V, ring):
    """Ear clipping of one ring: while ``m > 3`` the ``i`` with the smallest squared diagonal between
    ``r[i-1]`` and ``r[i+1]`` (a NaN counts as +inf; ties to the lowest ``i``) gives
    ``(r[i+1], r[i], r[i-1])`` and leaves; last ``(r[2], r[1], r[0])``."""
    r, out = list(ring), []
    while len(r) > 3:
        m = len(r)
        best, bd = 0, None
        for i in range(m):
            a, b = V[r[i - 1]], V[r[(i + 1) % m]]
            dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
            dd = (dx * dx + dy * dy) + dz * dz
            if not dd == dd:
                dd = np.inf
            if bd is None or dd < bd:
                best, bd = i, dd
        out.append((r[(best + 1) % m], r[best], r[best - 1]))
        del r[best]
    out.append((r[2], r[1], r[0]))
    return out


def close_holes(V, T, max_size=30):
    """``(triangles int32 [T + new, 3], record)``: the input triangles, then every closable loop's
    fill in ascending (leader, clip step)."""
    T = np.asarray(T, np.int32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        rec, loops = boundary_loops(T, len(V), max_size)
        new = [t for _, ring in loops for t in clip_ring(V, ring)]
    return np.concatenate([T, np.array(new, np.int32).reshape(-1, 3)]), rec


def postprocess(V, T, params):
    """``mesh.postprocess``: smoothing, then hole closing, from the reference's dict keys."""
    iters = int(params.get("smooth_iters", 10))
    V = smooth_laplacian(V, T, iters) if str(params.get("smooth_type", "taubin")) == "laplacian" else smooth_taubin(V, T, iters)
    if params.get("close_holes"):
        T = close_holes(V, T, int(params.get("close_max_size", 30)))[0]
    return V, np.asarray(T, np.int32)


def directed_unique(T):
    d = winding_pairs(T)
    return len(np.unique(d, axis=0)) == len(d)


# ------------------------------------------------------------------ mesh builders: (V float64 [n, 3], T int32 [m, 3])
def _mesh(V, T):
    return np.ascontiguousarray(V, np.float64).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3)


def tetrahedron():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


def octahedron():
    V = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    T = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return _mesh(V, T)


def single_triangle():
    return _mesh([[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5]], [[0, 1, 2]])


def grid_patch(nx, ny, z=None, seed=None):
    """A planar (or, with ``seed``, bumpy) patch of nx x ny quads, two triangles each, counter-clockwise
    seen from +z; vertex (i, j) has id j (nx + 1) + i."""
    X, Y = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64))
    Z = np.zeros_like(X) if seed is None else np.random.default_rng(seed).random(X.shape)
    V = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    T = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            b, c, d = a + 1, a + nx + 2, a + nx + 1
            T += [[a, b, c], [a, c, d]]
    return _mesh(V, T)


def open_strip(n=9):
    return grid_patch(n, 1)


def triangles_strip(nt):
    """Exactly ``nt`` triangles of a one-quad-high strip."""
    V, T = grid_patch((nt + 1) // 2, 1, seed=nt)
    return V, T[:nt].copy()


def disc_with_hole(L, outer=2.0, jitter=0.0, seed=0):
    """A planar annulus: an inner regular L-gon (radius 1) joined to an outer one; the inner ring is
    a hole of L edges, the outer boundary has L edges as well."""
    g = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(L) / L
    inner = np.stack([np.cos(ang), np.sin(ang), np.zeros(L)], axis=1)
    outer_v = outer * np.stack([np.cos(ang), np.sin(ang), np.zeros(L)], axis=1)
    V = np.concatenate([inner, outer_v]) + jitter * g.standard_normal((2 * L, 3))
    T = []
    for i in range(L):
        j = (i + 1) % L
        T += [[i, L + i, L + j], [i, L + j, j]]
    return _mesh(V, T)


def cone_with_hole(L, jitter=0.05, seed=0):
    """A disc with an L-gon hole whose outer boundary is closed by an apex fan on each side, so that
    the hole is the only boundary: a sphere with one punched hole of L edges."""
    V, T = disc_with_hole(L, jitter=jitter, seed=seed)
    apex = len(V)
    V = np.concatenate([V, [[0.0, 0.0, 3.0]]])
    T = list(map(list, T))
    for i in range(L):
        T.append([L + i, apex, L + (i + 1) % L])
    return _mesh(V, T)


def hexagon_hole():
    """A planar, point-symmetric hexagon hole with integer coordinates (a regular one has none): four
    of its six short diagonals have the squared length 13 exactly, the other two 16, so the tie rule
    decides the first clip."""
    inner = np.array([[2, 0, 0], [1, 2, 0], [-1, 2, 0], [-2, 0, 0], [-1, -2, 0], [1, -2, 0]], np.float64)
    V = np.concatenate([inner, 2.0 * inner])
    T = []
    for i in range(6):
        j = (i + 1) % 6
        T += [[i, 6 + i, 6 + j], [i, 6 + j, j]]
    return _mesh(V, T)


def bow_tie():
    """Two triangular holes that share vertex 4 of a 4 x 4 patch-like fan: the shared vertex has two
    outgoing boundary edges and is blocked."""
    V, T = grid_patch(4, 4, seed=3)
    drop = {(1, 1, 1), (2, 2, 0)}            # (i, j, which triangle of the quad): they meet at vertex (2, 2)
    keep = [k for k in range(len(T)) if ((k // 2) % 4, (k // 2) // 4, k % 2) not in drop]
    return V, T[keep].copy()


def unreferenced_vertex():
    V, T = octahedron()
    return np.concatenate([V[:3], [[9.0, 9.0, 9.0]], V[3:]]), np.where(T >= 3, T + 1, T).astype(np.int32)


def duplicated_triangle():
    V, T = grid_patch(3, 3, seed=5)
    return V, np.concatenate([T, T[7:8]])


def fan(n=80):
    """A closed fan around vertex 0: valence n, above the wave size."""
    ang = 2.0 * np.pi * np.arange(n) / n
    V = np.concatenate([[[0.0, 0.0, 0.5]], np.stack([np.cos(ang), np.sin(ang), 0.1 * np.cos(3 * ang)], axis=1)])
    return _mesh(V, [[0, 1 + i, 1 + (i + 1) % n] for i in range(n)])


def punched_lattice(nx=90, ny=60):
    """A bumpy patch with the quad (3 i + 1, 3 j + 1) of every 3 x 3 block removed: (nx / 3) (ny / 3)
    holes of 4 edges, 600 at the default size, whose 2,400 boundary edges and the outline's 300 fill
    eleven 256-thread workgroups."""
    V, T = grid_patch(nx, ny, seed=11)
    q = np.arange(len(T)) // 2
    keep = ~(((q % nx) % 3 == 1) & ((q // nx) % 3 == 1))
    return V, T[keep].copy()


@functools.lru_cache(maxsize=None)
def sphere_mesh(depth, seed, n=2000, trim=0.0):
    """``mesh_ref.extract`` of a ``mesh_ref.sphere`` cloud (with densities), after the density trim
    when ``trim > 0``.  Shared and read-only."""
    P, N = MR.sphere(n, seed)
    out = MR.poisson(P, N, depth)
    V, T, D = out["vertices"], out["triangles"], out["densities"]
    if trim > 0.0:
        V, T, D = MR.remove_vertices_by_mask(V, T, D, D < MR.quantile(D, trim))
    V, T, D = np.ascontiguousarray(V), np.ascontiguousarray(T, np.int32), np.ascontiguousarray(D)
    for a in (V, T, D):
        a.setflags(write=False)
    return V, T, D


# The depth-5 sphere cloud of the trimmed-mesh tests.  Of some 490 clouds searched (300 .. 16,000
# points, seeds 0 .. 109) this is the only one whose trimmed mesh closes without a repeated
# directed edge; tests/test_meshpost_ref.py:test_trimmed_sphere_closes says what that leaves.
TRIM_N, TRIM_SEED = 8000, 29


def trimmed_sphere():
    return sphere_mesh(5, TRIM_SEED, TRIM_N, 0.02)


BUILDERS = {
    "tetrahedron": tetrahedron, "octahedron": octahedron, "single_triangle": single_triangle, "open_strip": open_strip,
    "disc_hole5": lambda: disc_with_hole(5, jitter=0.05), "bow_tie": bow_tie, "unreferenced": unreferenced_vertex,
    "duplicated": duplicated_triangle, "fan": fan, "hexagon": hexagon_hole,
    "sphere4": lambda: sphere_mesh(4, 3, 500)[:2], "sphere5": lambda: sphere_mesh(5, TRIM_SEED, TRIM_N)[:2],
    "trimmed5": lambda: trimmed_sphere()[:2],
}
