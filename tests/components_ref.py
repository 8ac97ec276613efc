"""Connected components of a voxel grid as include/fidget_hip.h defines them (fhip_voxels_components), worked out on the unpacked
`inside[i, j, k]` bool array of voxels_ref.py - no bricks, no bit tricks, nothing of the library:

  offsets(conn)                 the 6 or 26 neighbour offsets
  keys(N)                       int64 [N, N, N]: the key of voxel (i, j, k), word_index * 64 + bit
  components(fg, conn)          Ref: labels int32 [N, N, N] (-1 background), count, sizes, seeds, lo, hi, border - numbered by
                                ascending seed key.  Union-find over the voxel pairs of the 3 or 13 positive offsets, the hooking and
                                the pointer jumping done for all pairs at once with numpy.
  components_bfs(fg, conn)      the same labels by a breadth-first search in plain Python, one voxel at a time (small grids): the two
                                are held to each other by tests/test_components.py; labels_bfs: its labels and count alone
  foreground(inside, complement)
"""
import collections
import functools

import numpy as np

Ref = collections.namedtuple("Ref", "labels count sizes seeds lo hi border")


def offsets(conn):
    assert conn in (6, 26)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = abs(dx) + abs(dy) + abs(dz)
                if n == 1 or (conn == 26 and n > 1):
                    out.append((dx, dy, dz))
    return out


@functools.lru_cache(maxsize=None)
def keys(N):
    """key[i, j, k] = ((bz B + by) B + bx) * 64 + lx + 4 ly + 16 lz with (i, j, k) = (4 bx + lx, 4 by + ly, 4 bz + lz), B = N / 4"""
    assert N % 4 == 0
    B = N // 4
    a = np.arange(N, dtype=np.int64)
    b, l = a // 4, a % 4
    i, j, k = np.meshgrid(a, a, a, indexing="ij")
    key = ((b[k] * B + b[j]) * B + b[i]) * 64 + l[i] + 4 * l[j] + 16 * l[k]
    key.setflags(write=False)          # (shared between calls)
    return key


def foreground(inside, complement=False):
    inside = np.asarray(inside, bool)
    return ~inside if complement else inside


def _table(labels, count, key):
    N = labels.shape[0]
    fg = labels >= 0
    lab = labels[fg].astype(np.int64)
    sizes = np.bincount(lab, minlength=count).astype(np.uint64)
    coords = np.stack(np.nonzero(fg), axis=1).astype(np.int64)         # [n, 3] (i, j, k)
    lo = np.full((count, 3), N, np.int64)
    hi = np.full((count, 3), -1, np.int64)
    seed_key = np.full(count, np.iinfo(np.int64).max, np.int64)
    kk = key[fg]
    for a in range(3):
        np.minimum.at(lo[:, a], lab, coords[:, a])
        np.maximum.at(hi[:, a], lab, coords[:, a])
    np.minimum.at(seed_key, lab, kk)
    seeds = np.zeros((count, 3), np.int64)
    at_seed = kk == seed_key[lab]
    seeds[lab[at_seed]] = coords[at_seed]
    on_border = ((coords == 0) | (coords == N - 1)).any(axis=1)
    border = np.zeros(count, bool)
    border[lab[on_border]] = True
    assert count == 0 or (np.diff(seed_key) > 0).all()          # numbered by ascending seed key
    return Ref(labels, count, sizes, seeds.astype(np.uint32), lo.astype(np.uint32), hi.astype(np.uint32), border)


def _cut(d, N):
    """the slices of a voxel and of its neighbour one step d along an axis"""
    return (slice(0, N - 1), slice(1, N)) if d == 1 else (slice(1, N), slice(0, N - 1)) if d == -1 else (slice(0, N), slice(0, N))


def components(fg, conn):
    fg = np.asarray(fg, bool)
    N = fg.shape[0]
    assert fg.shape == (N, N, N)
    key = keys(N)
    labels = np.full((N, N, N), -1, np.int32)
    n = int(fg.sum())
    if n == 0:
        return _table(labels, 0, key)
    # the foreground voxels in key order: voxel number v is the one with the v-th smallest key
    order = np.argsort(key[fg], kind="stable")
    number = np.full((N, N, N), -1, np.int64)
    flat = np.flatnonzero(fg.reshape(-1))
    number.reshape(-1)[flat[order]] = np.arange(n)
    pa, pb = [], []
    for dx, dy, dz in offsets(conn):
        if (dz, dy, dx) < (0, 0, 0):
            continue            # each pair once, from the positive half
        (x0, x1), (y0, y1), (z0, z1) = _cut(dx, N), _cut(dy, N), _cut(dz, N)
        a, b = number[x0, y0, z0], number[x1, y1, z1]
        both = (a >= 0) & (b >= 0)
        pa.append(a[both])
        pb.append(b[both])
    pa, pb = np.concatenate(pa), np.concatenate(pb)
    parent = np.arange(n)
    while True:
        ra, rb = parent[pa], parent[pb]          # (parent is fully compressed here: these are roots)
        differ = ra != rb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])        # hook the larger root to the smaller
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    roots = np.flatnonzero(parent == np.arange(n))           # ascending: the root is its component's voxel of smallest key
    comp = np.searchsorted(roots, parent)
    labels.reshape(-1)[flat[order]] = comp.astype(np.int32)
    return _table(labels, len(roots), key)


def labels_bfs(fg, conn):
    """-> labels, count"""
    fg = np.asarray(fg, bool)
    N = fg.shape[0]
    key = keys(N)
    labels = np.full((N, N, N), -1, np.int32)
    offs = offsets(conn)
    todo = sorted((int(key[i, j, k]), int(i), int(j), int(k)) for i, j, k in zip(*np.nonzero(fg)))
    count = 0
    for _, i, j, k in todo:          # ascending key: an unlabelled voxel met here is the seed of the next component
        if labels[i, j, k] >= 0:
            continue
        labels[i, j, k] = count
        queue = collections.deque([(i, j, k)])
        while queue:
            x, y, z = queue.popleft()
            for dx, dy, dz in offs:
                u, v, w = x + dx, y + dy, z + dz
                if 0 <= u < N and 0 <= v < N and 0 <= w < N and fg[u, v, w] and labels[u, v, w] < 0:
                    labels[u, v, w] = count
                    queue.append((u, v, w))
        count += 1
    return labels, count


def components_bfs(fg, conn):
    labels, count = labels_bfs(fg, conn)
    return _table(labels, count, keys(labels.shape[0]))
