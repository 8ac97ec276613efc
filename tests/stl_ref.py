"""Mesh::write_stl (fidget-mesh/src/output.rs:14-36) restated in numpy from the file format, for the tests of fhip_mesh_stl: 80 bytes
of header (the text, then zeros), the triangle count as a little-endian u32, then per triangle 50 bytes - the normal (b - a) x (c - a),
the corners a, b, c (little-endian f32 each) and two zero bytes.  Everything is float32 arrays, so every difference and every product
is rounded to f32 once, as the reference's f32 arithmetic rounds them; the cross product is x = u.y v.z - u.z v.y, y = u.z v.x - u.x v.z,
z = u.x v.y - u.y v.x.  The normal is not normalised."""
import numpy as np

HEADER_TEXT = b"This is a binary STL file exported by Fidget"


def stl_bytes(vertices, triangles):
    """(vertices [m, 3] float32, triangles [n, 3] vertex indices) -> the file as a uint8 array of 84 + 50 n bytes"""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    n = len(t)
    out = np.zeros(84 + 50 * n, np.uint8)
    out[:len(HEADER_TEXT)] = np.frombuffer(HEADER_TEXT, np.uint8)
    out[80:84] = np.frombuffer(np.array([n], "<u4").tobytes(), np.uint8)
    if n == 0:
        return out
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    u, w = b - a, c - a
    assert u.dtype == np.float32 and w.dtype == np.float32
    normal = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1],
                       u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                       u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    assert normal.dtype == np.float32
    rec = np.zeros((n, 50), np.uint8)
    rec[:, :48] = np.ascontiguousarray(np.concatenate([normal, a, b, c], axis=1).astype("<f4")).view(np.uint8).reshape(n, 48)
    out[84:] = rec.reshape(-1)
    return out
