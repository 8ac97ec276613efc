"""The boundary mesh of a voxel bitmap (fhip_voxels_mesh, fhip_voxels_surface; include/fidget_hip.h) restated in numpy on the unpacked
grid inside[i, j, k]: padded, shifted views and a sort on the stated keys - none of the bricks' bit arithmetic, so that the two check
each other.

  face     a set voxel and a direction d = 0 .. 5 = -x, +x, -y, +y, -z, +z in which its neighbour is clear (clear beyond the grid)
  corners  of a face, counter-clockwise seen from outside: with (u, v) the next two axes cyclically, o, o+u, o+u+v, o+v from
           o = voxel + e_a on the + side; o, o+v, o+u+v, o+u from o = voxel on the - side
  order    faces ascending by (brick word, d, bit in the brick); face f gives triangles 2f = (c0, c1, c2), 2f + 1 = (c0, c2, c3)
  vertex   a lattice corner whose eight voxels are not all equal; numbered ascending by (corner brick, local bit), the corner brick
           of (a, b, c) being ((c >> 2) (B + 1) + (b >> 2)) (B + 1) + (a >> 2) and the bit (a & 3) + 4 (b & 3) + 16 (c & 3)
  edge     a lattice edge whose four voxels are not all equal
"""
import numpy as np


def _grid(inside):
    inside = np.asarray(inside, bool)
    N = inside.shape[0]
    assert inside.shape == (N, N, N) and N % 4 == 0
    return inside, N, np.pad(inside, 1)


def faces(inside):
    """-> (voxel [F, 3], d [F]) in face order"""
    inside, N, pad = _grid(inside)
    B = N // 4
    vox, dirs = [], []
    for d in range(6):
        lo = [1, 1, 1]
        lo[d // 2] += 1 if d & 1 else -1
        neighbour = pad[lo[0]:lo[0] + N, lo[1]:lo[1] + N, lo[2]:lo[2] + N]
        at = np.argwhere(inside & ~neighbour)
        vox.append(at)
        dirs.append(np.full(len(at), d, np.int64))
    vox, dirs = np.concatenate(vox).astype(np.int64), np.concatenate(dirs)
    i, j, k = vox.T
    word = ((k >> 2) * B + (j >> 2)) * B + (i >> 2)
    bit = (i & 3) + 4 * (j & 3) + 16 * (k & 3)
    order = np.lexsort((bit, dirs, word))
    return vox[order], dirs[order]


def face_corners(vox, dirs):
    """-> [F, 4, 3] lattice corners"""
    out = np.zeros((len(vox), 4, 3), np.int64)
    for d in range(6):
        a = d // 2
        u, v = (a + 1) % 3, (a + 2) % 3
        e = np.eye(3, dtype=np.int64)
        steps = [0 * e[0], e[u], e[u] + e[v], e[v]] if d & 1 else [0 * e[0], e[v], e[u] + e[v], e[u]]
        sel = dirs == d
        o = vox[sel] + (e[a] if d & 1 else 0)
        for q in range(4):
            out[sel, q] = o + steps[q]
    return out


def corner_key(c, N):
    """lattice corners [..., 3] -> corner brick * 64 + bit: the vertices ascend by it"""
    S = N // 4 + 1
    a, b, cc = c[..., 0], c[..., 1], c[..., 2]
    return (((cc >> 2) * S + (b >> 2)) * S + (a >> 2)) * 64 + (a & 3) + 4 * (b & 3) + 16 * (cc & 3)


def used_corners(inside):
    """-> [V, 3] lattice corners in vertex order"""
    inside, N, pad = _grid(inside)
    n_set = np.zeros((N + 1,) * 3, np.int8)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                n_set += pad[dx:dx + N + 1, dy:dy + N + 1, dz:dz + N + 1]
    c = np.argwhere((n_set > 0) & (n_set < 8)).astype(np.int64)
    return c[np.argsort(corner_key(c, N), kind="stable")]


def used_edge_ends(inside):
    """-> per axis t the lower ends [E_t, 3] of the used lattice edges along t"""
    inside, N, pad = _grid(inside)
    ends = []
    for t in range(3):
        shape = [N + 1] * 3
        shape[t] = N                       # the edge from corner (a, b, c) one step along t: its lower end stays below N there
        n_set = np.zeros(shape, np.int8)
        for p in (0, 1):
            for q in (0, 1):
                lo = [p, q]
                lo.insert(t, 1)            # along t the voxel with the corner's own coordinate; one below and the same on the other two
                n_set += pad[lo[0]:lo[0] + shape[0], lo[1]:lo[1] + shape[1], lo[2]:lo[2] + shape[2]]
        ends.append(np.argwhere((n_set > 0) & (n_set < 4)).astype(np.int64))
    return ends


def used_edges(inside):
    """-> the number of used lattice edges along x, y, z"""
    return [len(e) for e in used_edge_ends(inside)]


def _set_bits(n_words, keys):
    """word * 64 + bit keys -> uint64 [n_words]"""
    out = np.zeros(n_words, np.uint64)
    np.bitwise_or.at(out, keys >> 6, np.uint64(1) << (keys & 63).astype(np.uint64))
    return out


def brick_face_masks(inside):
    """-> uint64 [B^3, 6]: per brick word and direction the voxels with an exposed face"""
    inside, N, _ = _grid(inside)
    B = N // 4
    vox, dirs = faces(inside)
    i, j, k = vox.T
    key = (((k >> 2) * B + (j >> 2)) * B + (i >> 2)) * 64 + (i & 3) + 4 * (j & 3) + 16 * (k & 3)
    return np.stack([_set_bits(B ** 3, key[dirs == d]) for d in range(6)], axis=1)


def corner_brick_masks(inside):
    """-> uint64 [(B + 1)^3, 4]: per corner brick the used corners and the used edges along x, y, z, an edge at its lower end"""
    inside, N, _ = _grid(inside)
    n = (N // 4 + 1) ** 3
    return np.stack([_set_bits(n, corner_key(c, N)) for c in [used_corners(inside)] + used_edge_ends(inside)], axis=1)


def mesh_and_summary(inside):
    """-> (vertices float32 [V, 3], triangles uint64 [2 F, 3], [faces -x, +x, -y, +y, -z, +z, V, E, F, n] as fhip_voxels_surface
    fills them)"""
    inside, N, _ = _grid(inside)
    vox, dirs = faces(inside)
    corners = used_corners(inside)
    keys = corner_key(corners, N)
    fk = corner_key(face_corners(vox, dirs), N)
    ids = np.searchsorted(keys, fk)
    assert len(fk) == 0 or (int(ids.max()) < len(keys) and np.array_equal(keys[ids], fk)), "a face's corner is no used corner"
    tris = np.empty((len(vox), 2, 3), np.uint64)
    tris[:, 0] = ids[:, [0, 1, 2]]
    tris[:, 1] = ids[:, [0, 2, 3]]
    verts = (2 * corners - N).astype(np.float32) * np.float32(1.0 / N)
    per_dir = np.bincount(dirs, minlength=6).tolist()
    return verts.reshape(-1, 3), tris.reshape(-1, 3), per_dir + [len(corners), sum(used_edges(inside)), sum(per_dir), int(inside.sum())]


def mesh(inside):
    return mesh_and_summary(inside)[:2]


def summary(inside):
    return mesh_and_summary(inside)[2]


def euler(s):
    return s[6] - s[7] + s[8]


def lattice(verts, N):
    """vertices of a mesh back in lattice units: exact integers"""
    return np.rint((np.asarray(verts, np.float64) * N + N) / 2).astype(np.int64)


def six_volumes(corners, tris):
    """the sum over the triangles of det(a, b, c), in lattice units: six times the enclosed volume"""
    p = corners[np.asarray(tris, np.int64)]
    return int(np.einsum("ni,ni->n", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum())


def edges_balanced(tris):
    """every directed edge occurs as often as its reverse"""
    t = np.asarray(tris, np.int64)
    if len(t) == 0:
        return True
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(e.max()) + 1
    fwd = np.sort(e[:, 0] * n + e[:, 1])
    rev = np.sort(e[:, 1] * n + e[:, 0])
    return bool(np.array_equal(fwd, rev))
