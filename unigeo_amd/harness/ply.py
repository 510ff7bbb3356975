"""Triangle meshes in PLY files: the reader the ScanNet++ renderer needs for ``scans/mesh_aligned_0.05.ply`` and a
writer for tests and tools.  No trimesh, no open3d: the header is parsed here and the body is read with numpy.

``read_ply_mesh`` takes binary little-endian and ASCII files, any scalar vertex properties of any PLY scalar type (``x``, ``y``, ``z`` are
picked by name, the others skipped), faces as ``property list uchar int|uint vertex_indices`` (also named ``vertex_index``), further elements
after the faces ignored.  Only triangles: a face with another vertex count is a ``ValueError``.  A file without a face element (a point cloud,
``harness.vis.write_ply``) gives an empty ``[0,3]`` face array."""
import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
          "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _header(raw, path):
    if not raw.startswith(b"ply"):
        raise ValueError(f"{path}: not a PLY file")
    end = raw.find(b"end_header")
    if end < 0:
        raise ValueError(f"{path}: PLY header without end_header")
    nl = raw.find(b"\n", end)
    if nl < 0:
        raise ValueError(f"{path}: PLY header without a closing line break")
    lines = [ln.strip() for ln in raw[:end].decode("ascii", "replace").splitlines()]
    fmt, elements = None, []                      # elements: [name, count, [(kind, name, type[, count type])]]
    for ln in lines[1:]:
        w = ln.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property":
            if not elements:
                raise ValueError(f"{path}: a property before any element")
            if w[1] == "list":
                elements[-1][2].append(("list", w[4], w[3], w[2]))
            else:
                elements[-1][2].append(("scalar", w[2], w[1]))
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (binary_little_endian, ascii)")
    for _, _, props in elements:
        for p in props:
            for ty in p[2:]:
                if ty not in _TYPES:
                    raise ValueError(f"{path}: unknown PLY type {ty!r}")
    return fmt, elements, nl + 1


def _xyz(cols, props, path):
    names = [p[1] for p in props]
    if not all(n in names for n in "xyz"):
        raise ValueError(f"{path}: the vertex element lacks x, y or z")
    return np.stack([np.asarray(cols[n]) for n in "xyz"], axis=1).astype(np.float32)


def _triangles(counts, path):
    if len(counts) and (counts != 3).any():
        raise ValueError(f"{path}: a face with {int(counts[counts != 3][0])} vertices; only triangles are supported")


def read_ply_mesh(path):
    """-> ``(verts float32 [NV,3], faces int32 [NF,3])``."""
    with open(path, "rb") as f:
        raw = f.read()
    fmt, elements, off = _header(raw, path)
    verts, faces = None, np.zeros((0, 3), np.int32)
    tokens = raw[off:].split() if fmt == "ascii" else None
    pos = 0
    for name, count, props in elements:
        lists = [p for p in props if p[0] == "list"]
        if name == "vertex":
            if lists:
                raise ValueError(f"{path}: a list property on the vertex element")
            if fmt == "ascii":
                n = count * len(props)
                if pos + n > len(tokens):
                    raise ValueError(f"{path}: the file ends inside the vertices")
                tab = np.array(tokens[pos:pos + n], dtype=np.float64).reshape(count, len(props)); pos += n
                cols = {p[1]: tab[:, i] for i, p in enumerate(props)}
            else:
                dt = np.dtype([(p[1], "<" + _TYPES[p[2]]) for p in props])
                if off + count * dt.itemsize > len(raw):
                    raise ValueError(f"{path}: the file ends inside the vertices")
                cols = np.frombuffer(raw, dt, count=count, offset=off); off += count * dt.itemsize
            verts = _xyz(cols, props, path)
        elif name == "face":
            if len(lists) != 1 or lists[0][1] not in ("vertex_indices", "vertex_index") or lists[0][3] not in ("uchar", "uint8") \
                    or lists[0][2] not in ("int", "int32", "uint", "uint32"):
                raise ValueError(f"{path}: faces must be one 'property list uchar int|uint vertex_indices'")
            li = props.index(lists[0])
            if fmt == "ascii":
                out = np.empty((count, 3), np.int64)
                for i in range(count):
                    row = []
                    for p in props:                          # scalars before or after the list are skipped
                        if p[0] == "list":
                            if pos >= len(tokens):
                                raise ValueError(f"{path}: the file ends inside the faces")
                            k = int(tokens[pos]); pos += 1
                            _triangles(np.array([k]), path)
                            row = tokens[pos:pos + k]; pos += k
                        else:
                            pos += 1
                    if len(row) != 3:
                        raise ValueError(f"{path}: the file ends inside the faces")
                    out[i] = [int(x) for x in row]
                faces = out
            else:
                # fixed-size records hold only if every face is a triangle: read them as such, then check every count
                dt = np.dtype([(f"s{i}", "<" + _TYPES[p[2]]) if p[0] == "scalar" else (f"s{i}", [("n", "u1"), ("v", "<" + _TYPES[p[2]], 3)])
                               for i, p in enumerate(props)])
                if off + count * dt.itemsize > len(raw):
                    # a short file, or a face that is no triangle: look at the first count that is not 3 to tell which
                    _triangles(_walk_counts(raw, off, count, props), path)
                    raise ValueError(f"{path}: the file ends inside the faces")
                rec = np.frombuffer(raw, dt, count=count, offset=off)
                if (rec[f"s{li}"]["n"] != 3).any():
                    _triangles(_walk_counts(raw, off, count, props), path)
                off += count * dt.itemsize
                faces = rec[f"s{li}"]["v"].astype(np.int64)
            if len(faces) and (faces.min() < 0 or faces.max() >= (1 << 31)):
                raise ValueError(f"{path}: a face index does not fit 31 bits")
            faces = np.ascontiguousarray(faces, dtype=np.int32)
        elif lists:
            break                                            # an element of unknown size: what follows it cannot be reached and is not needed
        elif fmt == "ascii":
            pos += count * len(props)
        else:
            off += count * sum(np.dtype(_TYPES[p[2]]).itemsize for p in props)
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    if len(faces) and faces.max() >= len(verts):
        raise ValueError(f"{path}: a face index lies outside the vertices")
    return verts, faces


def _walk_counts(raw, off, count, props):
    """The vertex counts of binary faces read one by one, up to and including the first that is not 3."""
    counts = []
    for _ in range(count):
        for p in props:
            if p[0] == "scalar":
                off += np.dtype(_TYPES[p[2]]).itemsize
            else:
                if off >= len(raw):
                    return np.array(counts, np.int64)
                k = raw[off]; off += 1 + k * np.dtype(_TYPES[p[2]]).itemsize
                counts.append(k)
                if k != 3:
                    return np.array(counts, np.int64)
    return np.array(counts, np.int64)


def write_ply_mesh(path, verts, faces, ascii=False):
    """float32 ``x y z`` per vertex and ``list uchar int vertex_indices`` per face, binary little-endian or ASCII (``%.9g``: a float32 survives)."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    head = (f"ply\nformat {'ascii' if ascii else 'binary_little_endian'} 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\n"
            f"property float z\nelement face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as out:
        out.write(head.encode("ascii"))
        if ascii:
            out.write("".join("%.9g %.9g %.9g\n" % tuple(r) for r in v.tolist()).encode("ascii"))
            out.write("".join("3 %d %d %d\n" % tuple(r) for r in f.tolist()).encode("ascii"))
        else:
            out.write(v.astype("<f4").tobytes())
            rec = np.empty(len(f), np.dtype([("n", "u1"), ("v", "<i4", 3)]))
            rec["n"], rec["v"] = 3, f
            out.write(rec.tobytes())
