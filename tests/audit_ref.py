"""NumPy restatement of the device mesh audit and cleanup (``csrc/cloud_audit.hip``):
edge classes, degenerate and duplicated triangles, connected components, vertex fans, signed volume
and area, and the selections built on them.  Plain loops and sorts wherever order matters; the
measures use ``+ - * /`` and ``sqrt`` in fp64 with every product and sum named and the additions in the
device's fixed shape, so the device is expected to equal these functions bit for bit.  Our rules:
parity with Open3D / MeshLab is unpinned.  Self-intersection is not tested.  Also the meshes the tests
are built from.
"""
import numpy as np

import meshpost_ref as P

CHUNK = 2048                      # triangles per partial sum (SLG_AUDIT_CHUNK): 256 threads of 8
REFERENCED, ON_BOUNDARY, ON_NONMANIFOLD_EDGE, ON_INCONSISTENT_EDGE, NONMANIFOLD_VERTEX = 1, 2, 4, 8, 16
DEGENERATE, DUPLICATE = 1, 2
COUNTS = ("vertices", "triangles", "unreferenced_vertices", "degenerate_triangles", "duplicate_triangles", "edges",
          "boundary_edges", "manifold_edges", "nonmanifold_edges", "inconsistent_edges", "nonmanifold_vertices", "components",
          "largest_component_triangles")
VERDICTS = ("closed", "edge_manifold", "vertex_manifold", "oriented", "watertight")


# ------------------------------------------------------------------ rules
def check_indices(T, nv):
    T = np.asarray(T, np.int64).reshape(-1, 3)
    if len(T) and (T.min() < 0 or T.max() >= nv):
        raise IndexError("a triangle index lies outside 0 .. V - 1")
    return T


def is_degenerate(T):
    T = np.asarray(T, np.int64).reshape(-1, 3)
    return (T[:, 0] == T[:, 1]) | (T[:, 1] == T[:, 2]) | (T[:, 2] == T[:, 0])


def edge_runs(T):
    """The runs of the stable sort: a list of ``(lo, hi, [(position 3 t + e, direction bit) ...])`` in
    ascending ``(lo, hi)``, each run's positions ascending.  Degenerate triangles give no entry."""
    T = np.asarray(T, np.int64).reshape(-1, 3)
    entries = []
    for t in np.flatnonzero(~is_degenerate(T)):
        for e in range(3):
            a, b = int(T[t, e]), int(T[t, (e + 1) % 3])
            entries.append((min(a, b), max(a, b), 3 * int(t) + e, 1 if a > b else 0))
    entries.sort(key=lambda x: (x[0], x[1]))                # Python's sort is stable
    runs = []
    for lo, hi, pos, d in entries:
        if runs and runs[-1][0] == lo and runs[-1][1] == hi:
            runs[-1][2].append((pos, d))
        else:
            runs.append((lo, hi, [(pos, d)]))
    return runs


class MinForest:
    """A union-find whose root is the smallest index of its set."""

    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        while self.parent[x] != x:
            self.parent[x] = self.parent[self.parent[x]]
            x = self.parent[x]
        return x

    def unite(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


def tree_sum(x):
    """The device's fixed shape over a vector: 8 consecutive terms per thread ``((0 + x0) + x1) + ..``,
    256 threads per chunk joined by the binary tree ``a[t] = a[t] + a[t + s]``, ``s = 128 .. 1``; then
    thread ``t`` adds the partials ``t, t + 256, ..`` in order from 0 and the same tree joins them."""
    x = np.asarray(x, np.float64)
    nb = max(1, -(-len(x) // CHUNK))
    a = np.zeros(nb * CHUNK)
    a[:len(x)] = x
    a = a.reshape(nb, 256, CHUNK // 256)
    s = np.zeros((nb, 256))
    for j in range(CHUNK // 256):
        s = s + a[:, :, j]
    part = _tree(s)
    rounds = -(-nb // 256)
    p = np.zeros(rounds * 256)
    p[:nb] = part
    p = p.reshape(rounds, 256)
    s = np.zeros((1, 256))
    for r in range(rounds):
        s = s + p[r][None, :]
    return float(_tree(s)[0])


def _tree(s):
    s = s.copy()
    w = 128
    while w > 0:
        s[:, :w] = s[:, :w] + s[:, w:2 * w]
        w //= 2
    return s[:, 0]


def measures(V, T):
    """``(signed_volume, area)``: the terms of the triangles that are not degenerate (a degenerate one
    adds nothing, which in the sums is a term of +0), summed by :func:`tree_sum`."""
    V, T = np.asarray(V, np.float64).reshape(-1, 3), np.asarray(T, np.int64).reshape(-1, 3)
    if len(T) == 0:
        return 0.0, 0.0
    a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    with np.errstate(all="ignore"):
        cx = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
        cy = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
        cz = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
        vol = ((a[:, 0] * cx + a[:, 1] * cy) + a[:, 2] * cz) / 6.0
        u, v = b - a, c - a
        nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
        live = ~is_degenerate(T)
        return tree_sum(np.where(live, vol, 0.0)), tree_sum(np.where(live, area, 0.0))


def verdict(counts):
    v = dict(closed=counts["boundary_edges"] == 0, edge_manifold=counts["nonmanifold_edges"] == 0,
             vertex_manifold=counts["nonmanifold_vertices"] == 0, oriented=counts["inconsistent_edges"] == 0)
    v["watertight"] = (all(v.values()) and counts["degenerate_triangles"] == 0 and counts["duplicate_triangles"] == 0
                       and counts["triangles"] > 0)
    return v


def audit(V, T):
    """``mesh.audit(..., return_arrays=True)`` as a dict of Python numbers and NumPy arrays."""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    nv = len(V)
    T = check_indices(T, nv)
    nt = len(T)
    res = dict.fromkeys(COUNTS, 0)
    res.update(vertices=nv, triangles=nt, unreferenced_vertices=nv, signed_volume=0.0, area=0.0,
               vertex_class=np.zeros(nv, np.uint8), triangle_class=np.zeros(nt, np.uint8), labels=np.full(nt, -1, np.int32),
               sizes=np.zeros(0, np.int64))
    if nv == 0 or nt == 0:
        res.update(verdict(res))
        return res
    deg = is_degenerate(T)
    vclass, tclass = res["vertex_class"], res["triangle_class"]
    tclass[deg] = DEGENERATE
    vclass[np.unique(T)] |= REFERENCED
    runs = edge_runs(T)
    tris, corners = MinForest(nt), MinForest(3 * nt)
    for lo, hi, run in runs:
        m = len(run)
        res["edges"] += 1
        bits = 0
        if m == 1:
            res["boundary_edges"] += 1
            bits |= ON_BOUNDARY
        elif m == 2:
            res["manifold_edges"] += 1
            if run[0][1] == run[1][1]:
                res["inconsistent_edges"] += 1
                bits |= ON_INCONSISTENT_EDGE
        else:
            res["nonmanifold_edges"] += 1
            bits |= ON_NONMANIFOLD_EDGE
        vclass[lo] |= bits
        vclass[hi] |= bits

        def corner(pos, d, at_max):
            t, e = divmod(pos, 3)
            return 3 * t + e if (d == 1) == at_max else 3 * t + (e + 1) % 3
        for k, (pos, d) in enumerate(run):
            t = pos // 3
            if k:
                tris.unite(t, run[0][0] // 3)
                corners.unite(corner(pos, d, False), corner(*run[0], False))
                corners.unite(corner(pos, d, True), corner(*run[0], True))
            third = int(T[t, (pos % 3 + 2) % 3])
            if third > hi:                                  # the edge between the triangle's two smallest indices
                if any(int(T[p // 3, (p % 3 + 2) % 3]) == third for p, _ in run[:k]):
                    tclass[t] |= DUPLICATE
    roots = [tris.find(t) if not deg[t] else -1 for t in range(nt)]
    rank = {r: i for i, r in enumerate(sorted({r for r in roots if r >= 0}))}
    res["labels"] = np.array([rank[r] if r >= 0 else -1 for r in roots], np.int32)
    res["sizes"] = np.bincount(res["labels"][res["labels"] >= 0], minlength=len(rank)).astype(np.int64)
    fans = [set() for _ in range(nv)]
    for t in np.flatnonzero(~deg):
        for j in range(3):
            fans[T[t, j]].add(corners.find(3 * int(t) + j))
    for v in range(nv):
        if len(fans[v]) > 1:
            vclass[v] |= NONMANIFOLD_VERTEX
    vol, area = measures(V, T)
    res.update(unreferenced_vertices=int((vclass & REFERENCED == 0).sum()), degenerate_triangles=int(deg.sum()),
               duplicate_triangles=int((tclass & DUPLICATE != 0).sum()), nonmanifold_vertices=int((vclass & 16 != 0).sum()),
               components=len(rank), largest_component_triangles=int(res["sizes"].max()) if len(rank) else 0,
               signed_volume=vol, area=area)
    res.update(verdict(res))
    return res


def connected_components(V, T):
    a = audit(V, T)
    return a["labels"], a["sizes"]


# ------------------------------------------------------------------ selections
def select(V, T, D, keep, drop_unreferenced=True):
    """The triangles with ``keep`` in input order, the vertices they use (or all) in input order,
    renumbered; densities carried."""
    V, T = np.asarray(V, np.float64).reshape(-1, 3), np.asarray(T, np.int32).reshape(-1, 3)
    Tk = T[np.asarray(keep, bool)]
    used = np.zeros(len(V), bool)
    if drop_unreferenced:
        used[Tk.reshape(-1)] = True
    else:
        used[:] = True
    new = np.cumsum(used) - 1
    return V[used], new[Tk].astype(np.int32).reshape(-1, 3), None if D is None else np.asarray(D, np.float64)[used]


def _by_components(V, T, D, choose):
    a = audit(V, T)
    table = np.asarray(choose(a["sizes"]), bool) if a["components"] else np.zeros(0, bool)
    keep = np.array([l >= 0 and table[l] for l in a["labels"]], bool)
    Vo, To, Do = select(V, T, D, keep)
    rec = dict(components_before=a["components"], components_after=int(table.sum()), triangles_removed=len(keep) - len(To),
               vertices_removed=len(np.asarray(V).reshape(-1, 3)) - len(Vo))
    return Vo, To, Do, rec


def keep_largest_components(V, T, D=None, count=1):
    def choose(sizes):
        table = np.zeros(len(sizes), bool)
        table[sorted(range(len(sizes)), key=lambda l: (-int(sizes[l]), l))[:count]] = True
        return table
    return _by_components(V, T, D, choose)


def remove_small_components(V, T, D=None, min_triangles=0):
    return _by_components(V, T, D, lambda sizes: sizes >= min_triangles)


def clean(V, T, D=None, degenerate=True, duplicates=True, unreferenced=True):
    a = audit(V, T)
    drop = (DEGENERATE if degenerate else 0) | (DUPLICATE if duplicates else 0)
    keep = (a["triangle_class"] & drop) == 0
    Vo, To, Do = select(V, T, D, keep, unreferenced)
    rec = dict(degenerate_removed=a["degenerate_triangles"] if degenerate else 0,
               duplicates_removed=a["duplicate_triangles"] if duplicates else 0, vertices_removed=a["vertices"] - len(Vo))
    return Vo, To, Do, rec


def postprocess(V, T, D, params):
    """``mesh.postprocess`` with the keys of §22 (without ``simplify``): ``(V, T, D, audit or None)``."""
    if params.get("keep_components") is not None:
        V, T, D, _ = keep_largest_components(V, T, D, int(params["keep_components"]))
    if params.get("min_component_faces") is not None:
        V, T, D, _ = remove_small_components(V, T, D, int(params["min_component_faces"]))
    V, T = P.postprocess(V, T, params)
    if params.get("clean"):
        V, T, D, _ = clean(V, T, D)
    return V, T, D, (audit(V, T) if params.get("audit") else None)


# ------------------------------------------------------------------ meshes: (V float64 [n, 3], T int32 [m, 3])
def book(pages, repeat=()):
    """``pages`` triangles on the edge (0, 1), page ``k`` with the third vertex ``2 + k`` and the winding
    alternating; the pages in ``repeat`` come a second time at the end, wound the other way."""
    ang = 2.0 * np.pi * np.arange(pages) / pages
    V = np.concatenate([[[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], np.stack([np.cos(ang), np.sin(ang), 0.5 + 0.0 * ang], axis=1)])
    T = [[0, 1, 2 + k] if k % 2 == 0 else [1, 0, 2 + k] for k in range(pages)]
    T += [[1, 0, 2 + k] if k % 2 == 0 else [0, 1, 2 + k] for k in repeat]
    return P._mesh(V, T)


def two_tetrahedra(shared):
    """Two tetrahedra that share ``shared`` vertices: 1 (a pinch), 2 (an edge with four triangles)."""
    V1, T1 = P.tetrahedron()
    V2 = V1 * -1.0 if shared == 1 else np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float64)
    remap = {1: [0, 4, 5, 6], 2: [0, 1, 4, 5]}[shared]
    T2 = np.array(remap, np.int32)[T1]
    if shared == 1:
        T2 = T2[:, ::-1]                                    # the point reflection turned it inside out
    V = np.concatenate([V1, V2[[k for k in range(4) if remap[k] >= 4]]])
    return P._mesh(V, np.concatenate([T1, T2]))


def moebius(n=12):
    """A Möbius strip of ``n`` quads: two rows of vertices, the last quad joined with a twist."""
    ang = 2.0 * np.pi * np.arange(n) / n
    ring = []
    for side in (-0.3, 0.3):
        r = 1.0 + side * np.cos(ang / 2.0)
        ring.append(np.stack([r * np.cos(ang), r * np.sin(ang), side * np.sin(ang / 2.0)], axis=1))
    V = np.concatenate(ring)
    T = []
    for i in range(n):
        a, b = i, n + i
        c, d = (i + 1, n + i + 1) if i + 1 < n else (n, 0)      # the twist: the rows swap at the seam
        T += [[a, c, d], [a, d, b]]
    return P._mesh(V, T)


def disjoint_tetrahedra(count=1000):
    """``count`` tetrahedra side by side, their triangles interleaved: face ``j`` of every tetrahedron
    comes before face ``j + 1`` of any, so a component's triangles lie ``count`` apart."""
    V0, T0 = P.tetrahedron()
    V = np.concatenate([V0 + [2.0 * k, 0.0, 0.0] for k in range(count)])
    T = np.concatenate([T0[j][None, :] + 4 * np.arange(count)[:, None] for j in range(4)])
    return P._mesh(V, T)


def octahedron_variant(kind):
    V, T = P.octahedron()
    if kind == "flipped":
        T = T.copy()
        T[3] = T[3, ::-1]
    elif kind == "degenerate":
        T = np.concatenate([T, [[2, 2, 4], [3, 3, 3]]])
    elif kind == "repeated":                                # face 2 again in both windings
        T = np.concatenate([T, T[2:3, ::-1], T[2:3]])
    elif kind == "reversed_repeat":
        T = np.concatenate([T, T[2:3, ::-1]])
    return P._mesh(V, T)


def reordered_strip(nt, order):
    V, T = P.triangles_strip(nt)
    idx = np.arange(nt)[::-1] if order == "reversed" else np.random.default_rng(nt).permutation(nt)
    return V, np.ascontiguousarray(T[idx])


BUILDERS = {
    **{k: v for k, v in P.BUILDERS.items() if k != "sphere4"},
    "one_vertex": lambda: (np.array([[1.0, 2.0, 3.0]]), np.zeros((0, 3), np.int32)),
    **{f"strip{n}": (lambda n=n: P.triangles_strip(n)) for n in (1, 85, 86, 256, 257)},
    "strip20000_reversed": lambda: reordered_strip(20000, "reversed"),
    "strip20000_shuffled": lambda: reordered_strip(20000, "shuffled"),
    "tetrahedra1000": disjoint_tetrahedra,
    "book3": lambda: book(3), "book80": lambda: book(80, repeat=(0, 5, 5, 63, 79)),
    "two_tetrahedra_vertex": lambda: two_tetrahedra(1), "two_tetrahedra_edge": lambda: two_tetrahedra(2),
    "moebius": moebius,
    "octahedron_flipped": lambda: octahedron_variant("flipped"), "octahedron_degenerate": lambda: octahedron_variant("degenerate"),
    "octahedron_repeated": lambda: octahedron_variant("repeated"),
    **{f"chunk{n}": (lambda n=n: P.triangles_strip(n)) for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)},
}
