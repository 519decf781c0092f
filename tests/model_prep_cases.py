"""Meshes and PLY files for the model-preparation tests, made in numpy: a subdivided icosahedron, a unit cube, a two-triangle strip."""
import zlib

import numpy as np


def seed_of(name):
    return zlib.crc32(name.encode())


def icosphere(subdivisions=3, radius=50.0):
    """(verts f64[V,3], faces i32[F,3]): 12 / 42 / 162 / 642 vertices and 20 / 80 / 320 / 1280 faces for 0 / 1 / 2 / 3 subdivisions."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
             (-t, 0, -1), (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in verts]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts) * radius, np.array(faces, dtype=np.int32)


def sphere_attributes(verts):
    """Outward unit normals f32[V,3] and position-dependent colours u8[V,3] that reach 0 and 255."""
    unit = verts / np.linalg.norm(verts, axis=1, keepdims=True)
    colors = np.clip(np.rint((unit * 0.5 + 0.5) * 300.0 - 20.0), 0, 255).astype(np.uint8)
    return unit.astype(np.float32), colors


def cube():
    """The unit cube, vertex i = (i >> 2 & 1, i >> 1 & 1, i & 1), 12 triangles."""
    verts = np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)], dtype=np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([f for a, b, c, d in quads for f in ((a, b, c), (a, c, d))], dtype=np.int32)
    return verts, faces


def strip():
    """Two triangles of area 3 : 1 in the tilted plane z = x / 2 + y / 4, sharing the edge 1-2."""
    xy = np.array([[0, 0], [3, 0], [0, 2], [2.5, 1]], dtype=np.float64)
    verts = np.concatenate([xy, xy[:, :1] * 0.5 + xy[:, 1:] * 0.25], axis=1)
    return verts, np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)


def write_ply(path, verts, faces, normals=None, colors=None, binary=False):
    props = ["float x", "float y", "float z"]
    if normals is not None:
        props += ["float nx", "float ny", "float nz"]
    if colors is not None:
        props += ["uchar red", "uchar green", "uchar blue"]
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment made by the tests",
            "element vertex %d" % len(verts)] + ["property " + p for p in props] + \
           ["element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if binary:
            dt = [(p.split()[1], "<f4" if p.startswith("float") else "u1") for p in props]
            rec = np.zeros(len(verts), dtype=dt)
            for k, nm in enumerate("xyz"):
                rec[nm] = verts[:, k]
            if normals is not None:
                for k, nm in enumerate(("nx", "ny", "nz")):
                    rec[nm] = normals[:, k]
            if colors is not None:
                for k, nm in enumerate(("red", "green", "blue")):
                    rec[nm] = colors[:, k]
            f.write(rec.tobytes())
            frec = np.zeros(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
            frec["n"], frec["v"] = 3, faces
            f.write(frec.tobytes())
        else:
            for i in range(len(verts)):
                row = ["%.9g" % v for v in np.asarray(verts[i], dtype=np.float32)]
                if normals is not None:
                    row += ["%.9g" % v for v in normals[i]]
                if colors is not None:
                    row += ["%d" % v for v in colors[i]]
                f.write((" ".join(row) + "\n").encode())
            for a, b, c in faces:
                f.write(("3 %d %d %d\n" % (a, b, c)).encode())
    return str(path)
