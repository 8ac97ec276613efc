"""The numpy model of 2D contouring, written from the definition in include/fidget_hip.h (fhip_contour2d) and from nothing else: plain
loops over lattice edges and cells, float32 scalars, a table typed in from the definition's.  It takes any [H, W] float32 image; the
tests compare the library's host build and the device with it, and hold it to properties that do not use the table."""
import numpy as np

NONE = 0xFFFFFFFF
f32 = np.float32

# mask -> segments as (from, to) edge letters; the inside on the left, x to the right, j upward
TABLE = {
    0: [], 15: [],
    1: [("B", "L")], 14: [("L", "B")],
    2: [("R", "B")], 13: [("B", "R")],
    4: [("T", "R")], 11: [("R", "T")],
    8: [("L", "T")], 7: [("T", "L")],
    3: [("R", "L")], 12: [("L", "R")],
    6: [("T", "B")], 9: [("B", "T")],
}
SADDLE = {  # (mask, centre inside)
    (5, True): [("B", "R"), ("T", "L")], (5, False): [("B", "L"), ("T", "R")],
    (10, True): [("L", "B"), ("R", "T")], (10, False): [("R", "B"), ("L", "T")],
}


def inside(v):
    return bool(v < 0)           # (NaN: False)


def contours(img):
    """-> dict: vertices [n, 2] float32, segments [m, 2] uint32, next [n] uint32, edge_of [n] (kind 'h' / 'u', i, j) per vertex,
    cell_of [m] (i, j) per segment, hist {(mask, centre inside or None): cells}, t_half: vertices placed by the t = 0.5 rule"""
    img = np.ascontiguousarray(img, np.float32)
    H, W = img.shape
    ins = [[inside(v) for v in row] for row in img.tolist()]        # (plain lists: a large image's loops stay quick)
    ids, verts, edge_of, t_half = {}, [], [], 0

    def vertex(kind, i, j):
        nonlocal t_half
        a, b = (img[j, i], img[j, i + 1]) if kind == "h" else (img[j, i], img[j + 1, i])
        with np.errstate(all="ignore"):
            t = f32(a) / f32(f32(a) - f32(b))
        if not (t >= 0 and t <= 1):
            t = f32(0.5)
            t_half += 1
        ids[(kind, i, j)] = len(verts)
        verts.append((f32(i) + t, f32(j)) if kind == "h" else (f32(i), f32(j) + t))
        edge_of.append((kind, i, j))

    for j in range(H):
        row = ins[j]
        for i in range(W - 1):
            if row[i] != row[i + 1]:
                vertex("h", i, j)
    for j in range(H - 1):
        row, up = ins[j], ins[j + 1]
        for i in range(W):
            if row[i] != up[i]:
                vertex("u", i, j)

    segs, cell_of, hist = [], [], {}
    nxt = np.full(len(verts), NONE, np.uint32)
    for j in range(H - 1):
        for i in range(W - 1):
            mask = ins[j][i] | ins[j][i + 1] << 1 | ins[j + 1][i + 1] << 2 | ins[j + 1][i] << 3
            centre = None
            if mask in (5, 10):
                v00, v10, v11, v01 = img[j, i], img[j, i + 1], img[j + 1, i + 1], img[j + 1, i]
                with np.errstate(all="ignore"):
                    centre = bool(f32(f32(f32(v00) + f32(v10)) + f32(f32(v11) + f32(v01))) * f32(0.25) < 0)
                pairs = SADDLE[(mask, centre)]
            else:
                pairs = TABLE[mask]
            hist[(mask, centre)] = hist.get((mask, centre), 0) + 1
            if not pairs:
                continue
            edge = {"B": ("h", i, j), "R": ("u", i + 1, j), "T": ("h", i, j + 1), "L": ("u", i, j)}
            for a, b in pairs:
                fr, to = ids[edge[a]], ids[edge[b]]
                assert nxt[fr] == NONE
                segs.append((fr, to))
                cell_of.append((i, j))
                nxt[fr] = to
    return {"vertices": np.array(verts, np.float32).reshape(-1, 2), "segments": np.array(segs, np.uint32).reshape(-1, 2), "next": nxt,
            "edge_of": edge_of, "cell_of": cell_of, "hist": hist, "t_half": t_half}


def loops(nxt):
    """[(ids, closed)]: open chains first, from the vertices nothing arrives at in ascending order; then closed loops, each from its
    smallest id, in ascending order of that"""
    nxt = [int(v) for v in nxt]
    has_in = set(v for v in nxt if v != NONE)
    done, out = set(), []
    for k in range(len(nxt)):
        if k in has_in:
            continue
        chain, v = [], k
        while v != NONE:
            chain.append(v)
            done.add(v)
            v = nxt[v]
        out.append((chain, False))
    for k in range(len(nxt)):
        if k in done:
            continue
        chain, v = [], k
        while v not in done:
            chain.append(v)
            done.add(v)
            v = nxt[v]
        assert v == k
        out.append((chain, True))
    return out


def area(vertices, ids):
    """the shoelace sum in float64"""
    p = np.asarray(vertices, np.float64)[list(ids)]
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
