"""NumPy restatement of the banded cascadic mesher (``csrc/cloud_band.hip``), built on
``mesh_ref`` with dense arrays plus masks: one function per rule, fp64, every sum in the order the
kernels take it, so the device is expected to equal these functions bit for bit.  Everything not
restated here is §16's rule, called from ``mesh_ref``.  Dense arrays make it feasible up to depth 7
(2 M nodes, a few seconds).

Arrays are indexed ``[z, y, x]`` as in ``mesh_ref``.  A block is 8^3 cells; block ``b`` owns the
nodes ``[8 b, 8 b + 8)`` per axis, so the nodes of an ``R``-cell level fall into ``(R / 8 + 1)^3``
node blocks (the last one per axis holds the box's far face alone).
"""
import numpy as np

import mesh_ref as M

B = 8
DEFAULT_BAND_SWEEPS = 16
MIN_DEPTH, MAX_DEPTH, MAX_BASE = 3, 12, 10


def default_base(depth):
    return min(8, depth - 1)


# ------------------------------------------------------------------ blocks, cells, nodes
def block_sets(P, origin, h, R):
    """``(seeded, active)``, bool ``[nb]^3``: a block is seeded when a point's cell lies in it and
    active when it or one of its 26 neighbours inside the grid is seeded."""
    nb = max(R // B, 1)
    i, _ = M.cell_of(P, origin, h, R)
    b = i // B
    seeded = np.zeros((nb, nb, nb), bool)
    seeded[b[:, 2], b[:, 1], b[:, 0]] = True
    pad = np.pad(seeded, 1)
    active = np.zeros_like(seeded)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                active |= pad[dz:dz + nb, dy:dy + nb, dx:dx + nb]
    return seeded, active


def cells_of_blocks(active, R):
    w = min(B, R)
    return np.repeat(np.repeat(np.repeat(active, w, axis=0), w, axis=1), w, axis=2)


def active_cells(P, origin, h, R):
    """bool ``[R]^3``: a cell is active when its block is."""
    return cells_of_blocks(block_sets(P, origin, h, R)[1], R)


def incident(cells):
    """uint8 ``[R+1]^3``: bit ``ex + 2 ey + 4 ez`` of a node is set when the cell at ``node - 1 + e`` is
    active (a cell outside the grid is not)."""
    n1 = cells.shape[0] + 1
    pad = np.pad(cells, 1)
    m = np.zeros((n1, n1, n1), np.uint8)
    for ez in (0, 1):
        for ey in (0, 1):
            for ex in (0, 1):
                m |= pad[ez:ez + n1, ey:ey + n1, ex:ex + n1].astype(np.uint8) << (ex + 2 * ey + 4 * ez)
    return m


def band_nodes(cells):
    """At least one incident cell is active."""
    return incident(cells) != 0


def interior_nodes(cells):
    """All 8 incident cells are active (so the node is not on the box boundary)."""
    return incident(cells) == 255


def node_blocks(active):
    """bool ``[nb+1]^3``: the node blocks that hold a band node: block ``b`` when one of the cell blocks
    ``b - {0, 1}^3`` is active."""
    nb = active.shape[0]
    out = np.zeros((nb + 1,) * 3, bool)
    for ez in (0, 1):
        for ey in (0, 1):
            for ex in (0, 1):
                out[ez:ez + nb, ey:ey + nb, ex:ex + nb] |= active
    return out


def blocked(field, nblocks):
    """A dense node field as the device stores it: ``[count, 8, 8, 8(, k)]``, the node blocks of
    ``nblocks`` in ascending id ``(bz (nb+1) + by) (nb+1) + bx``, nodes past the grid as 0."""
    nbk = nblocks.shape[0]
    full = np.zeros((B * nbk,) * 3 + field.shape[3:], field.dtype)
    n1 = field.shape[0]
    full[:n1, :n1, :n1] = field
    tail = field.shape[3:]
    v = full.reshape((nbk, B, nbk, B, nbk, B) + tail)
    v = v.transpose((0, 2, 4, 1, 3, 5) + tuple(range(6, 6 + len(tail))))
    return np.ascontiguousarray(v[nblocks])


# ------------------------------------------------------------------ one banded level
def level_solve(P, Nrm, origin, h, R, chi_parent, sweeps=DEFAULT_BAND_SWEEPS):
    """The level of ``R`` cells from its parent's solution (a dense ``[R/2+1]^3`` array whose values
    outside the parent's band are never read): a dict of every stage."""
    seeded, active = block_sets(P, origin, h, R)
    cells = cells_of_blocks(active, R)
    inc = incident(cells)
    band, inter = inc != 0, inc == 255
    W, V = M.splat(P, Nrm, origin, h, R)                      # inactive cells hold no points: the dense values
    f = np.where(inter, M.divergence(V, h), 0.0)
    u0 = np.where(band, 0.125 * M.prolong_add(np.zeros((R + 1,) * 3), chi_parent), 0.0)
    u, h2 = u0, h * h
    for _ in range(int(sweeps)):
        u = np.where(inter, M.smooth(u, f, h2), u)
    return dict(R=R, h=h, seeded=seeded, active=active, cells=cells, incident=inc, W=W, V=V, f=f, u0=u0, chi=u,
                record=dict(level=int(R).bit_length() - 1, seeded_blocks=int(seeded.sum()), active_blocks=int(active.sum()),
                            node_blocks=int(node_blocks(active).sum()), band_nodes=int(band.sum()),
                            interior_nodes=int(inter.sum())))


# ------------------------------------------------------------------ the surface inside the band
def _edge_active(inc, dx, dy, dz):
    """The owned edge (node, +d) lies in an active cell: one of the incident cells ``node - 1 + e``
    with ``e = 1`` on every axis the edge runs along."""
    out = np.zeros(inc.shape, bool)
    for ez in (0, 1):
        for ey in (0, 1):
            for ex in (0, 1):
                if ex >= dx and ey >= dy and ez >= dz:
                    out |= ((inc >> (ex + 2 * ey + 4 * ez)) & 1).astype(bool)
    return out


def extract_band(chi, iso, origin, h, W, cells):
    """``(vertices, triangles, densities)``: marching tetrahedra over the active cells only; an owned
    edge carries a vertex when it crosses and lies in an active cell.  Vertices in ascending (block,
    local node, edge type), triangles in ascending (block, local cell, tetrahedron, triangle)."""
    n1 = chi.shape[0]
    R = n1 - 1
    nbk = max(R // B, 1) + 1
    inc = incident(cells)
    inside = chi < iso
    mask = np.zeros((n1, n1, n1), np.uint8)
    for e, (dx, dy, dz) in enumerate(M.EDGE_OFF):
        a = inside[:n1 - dz, :n1 - dy, :n1 - dx]
        b = inside[dz:, dy:, dx:]
        ok = _edge_active(inc, dx, dy, dz)[:n1 - dz, :n1 - dy, :n1 - dx]
        mask[:n1 - dz, :n1 - dy, :n1 - dx] |= (((a != b) & ok).astype(np.uint8) << e)
    mflat = mask.ravel()
    cnt = M._popcount(mflat)
    vbase = np.cumsum(cnt) - cnt                           # dense ids: ascending (node, type)
    bits = (mflat[:, None] >> np.arange(7)[None, :]) & 1
    node, et = np.nonzero(bits)
    ia = np.stack([node % n1, (node // n1) % n1, node // (n1 * n1)], axis=1)

    def block_key(x, y, z):
        return ((((z // B) * nbk + y // B) * nbk + x // B) * B ** 3) + ((z % B) * B + y % B) * B + x % B
    order = np.argsort(block_key(ia[:, 0], ia[:, 1], ia[:, 2]) * 7 + et, kind="stable")
    newid = np.empty(len(order), np.int64)
    newid[order] = np.arange(len(order))
    node, et, ia = node[order], et[order], ia[order]
    ib = ia + np.array(M.EDGE_OFF, np.int64)[et]
    cf = chi.ravel()
    ca = cf[node]
    cb = cf[(ib[:, 2] * n1 + ib[:, 1]) * n1 + ib[:, 0]]
    t = (iso - ca) / (cb - ca)
    pa = origin[None, :] + h * ia.astype(np.float64)
    pb = origin[None, :] + h * ib.astype(np.float64)
    verts = pa + t[:, None] * (pb - pa)
    dens = M.sample(W, verts, origin, h) if W is not None and len(verts) else (np.zeros(0) if W is not None else None)
    zz, yy, xx = np.nonzero(cells)
    out_key, out_tri = [], []
    for k in range(6):
        corners = M.tet_corners(k)
        nodes = [((zz + c[2]) * n1 + (yy + c[1])) * n1 + (xx + c[0]) for c in corners]
        m = sum(inside.ravel()[nodes[v]].astype(np.int64) << v for v in range(4))
        for case in range(1, 15):
            s = np.flatnonzero(m == case)
            if not len(s):
                continue
            for j, tri in enumerate(M.tet_case(case, M.TET_ODD[k])):
                ids = []
                for p, q in tri:
                    d = [corners[q][a] - corners[p][a] for a in range(3)]
                    ty = M.EDGE_TYPE[d[0] + 2 * d[1] + 4 * d[2]]
                    owner = nodes[p][s]
                    ids.append(newid[vbase[owner] + M._popcount(mflat[owner] & ((1 << ty) - 1))])
                out_tri.append(np.stack(ids, axis=1))
                out_key.append((block_key(xx[s], yy[s], zz[s]) * 6 + k) * 2 + j)
    if out_tri:
        key = np.concatenate(out_key)
        tris = np.concatenate(out_tri)[np.argsort(key, kind="stable")].astype(np.int32)
    else:
        tris = np.zeros((0, 3), np.int32)
    return verts, tris, dens


# ------------------------------------------------------------------ the whole mesher
def check_depths(depth, base_depth=None):
    depth = int(depth)
    if not MIN_DEPTH <= depth <= MAX_DEPTH:
        raise ValueError("depth")
    base = default_base(depth) if base_depth is None else int(base_depth)
    if not 2 <= base <= min(MAX_BASE, depth - 1):
        raise ValueError("base_depth")
    return depth, base


def poisson_band(P, Nrm, depth, base_depth=None, sweeps=DEFAULT_BAND_SWEEPS, scale=1.1, cycles=M.DEFAULT_CYCLES):
    """The whole mesher: a dict of every stage's result; ``levels`` holds :func:`level_solve`'s dict
    of every banded level, coarsest first."""
    depth, base = check_depths(depth, base_depth)
    origin, h, R = M.grid(P, base, scale)
    Wb, Vb = M.splat(P, Nrm, origin, h, R)
    fb = M.divergence(Vb, h)
    chi = chi_base = M.solve(fb, h, cycles)
    levels = []
    for l in range(base + 1, depth + 1):
        origin, h, R = M.grid(P, l, scale)
        levels.append(level_solve(P, Nrm, origin, h, R, chi, sweeps))
        chi = levels[-1]["chi"]
    top = levels[-1]
    iso = M.iso_value(chi, P, origin, h)
    verts, tris, dens = extract_band(chi, iso, origin, h, top["W"], top["cells"])
    return dict(origin=origin, h=h, R=R, base=dict(W=Wb, V=Vb, f=fb, chi=chi_base), levels=levels, iso=iso,
                vertices=verts, triangles=tris, densities=dens, triangle_normals=M.triangle_normals(verts, tris),
                record=[lv["record"] for lv in levels])


def nested(levels):
    """The parent cell of every active cell of a level is active one level down (the first banded
    level's parent is the dense base)."""
    for lo, hi in zip(levels, levels[1:]):
        z, y, x = np.nonzero(hi["cells"])
        if not lo["cells"][z // 2, y // 2, x // 2].all():
            return False
    return True


def open_sphere(n, seed=1, cut=0.6):
    P, Nrm = M.sphere(n, seed)
    keep = P[:, 2] < cut
    return np.ascontiguousarray(P[keep]), np.ascontiguousarray(Nrm[keep])
