"""texture_mesh's host half (graph_utils.cpp:449-501): the coloured-PCD reader, the OBJ reader and the PLY writer of slam_wrapper
(_read_rgb_pcd / _read_obj / _write_mesh_ply), and texture_mesh's refusals, which all come before any device work.  No device needed."""
import os

import numpy as np
import pytest


def _module():
    import slam_wrapper

    assert slam_wrapper.__file__.endswith(".so")
    return slam_wrapper


def _same(a, b):
    """bit for bit, except that a NaN is a NaN whatever its payload (both sides' NaNs must sit in the same places)"""
    a, b = np.array(a, np.float32), np.array(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    a[np.isnan(a)] = 0
    b[np.isnan(b)] = 0
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


_NP = {("F", 4): "<f4", ("F", 8): "<f8", ("U", 1): "u1", ("U", 2): "<u2", ("U", 4): "<u4", ("U", 8): "<u8", ("I", 1): "i1", ("I", 2): "<i2",
       ("I", 4): "<i4", ("I", 8): "<i8"}


def _write_pcd(path, spec, cols, n, data, header_points=True):
    """spec: [(name, size, type, count)], cols: name -> array (n,) or (n, count) of the field's dtype"""
    head = ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7",
            "FIELDS " + " ".join(s[0] for s in spec), "SIZE " + " ".join(str(s[1]) for s in spec),
            "TYPE " + " ".join(s[2] for s in spec), "COUNT " + " ".join(str(s[3]) for s in spec),
            f"WIDTH {n}", "HEIGHT 1", "VIEWPOINT 0 0 0 1 0 0 0"]
    if header_points:
        head.append(f"POINTS {n}")
    head.append(f"DATA {data}")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if data == "binary":
            dt = np.dtype([(s[0], _NP[(s[2], s[1])], (s[3],)) if s[3] > 1 else (s[0], _NP[(s[2], s[1])]) for s in spec])
            rec = np.zeros(n, dt)
            for s in spec:
                rec[s[0]] = cols[s[0]]
            f.write(rec.tobytes())
        else:
            lines = []
            for i in range(n):
                toks = []
                for s in spec:
                    v = np.asarray(cols[s[0]][i]).reshape(-1)
                    toks += [repr(float(t)) if s[2] == "F" else str(int(t)) for t in v]
                lines.append(" ".join(toks))
            f.write(("\n".join(lines) + "\n").encode())


def _cloud_cols(n, rng, colour_type):
    xyz = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    xyz[rng.choice(n, n // 10, replace=False), rng.integers(0, 3)] = np.nan  # NaN rows are kept
    a = rng.integers(0, 0x7F, n).astype(np.uint32)  # alpha below 0x7F: as a float the word is never a NaN (ascii F round-trips)
    rgb = (a << 24) | rng.integers(0, 1 << 24, n).astype(np.uint32)
    cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2]}
    cols["rgb" if colour_type != "rgba" else "rgba"] = rgb.view(np.float32) if colour_type == "F" else rgb
    cols["b1"] = rng.integers(0, 255, n).astype(np.uint8)
    cols["s2"] = rng.integers(-3000, 3000, n).astype(np.int16)
    cols["w4"] = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    cols["d8"] = rng.uniform(-1, 1, n)
    cols["u8"] = rng.integers(0, 1 << 40, (n, 2)).astype(np.uint64)
    return xyz, rgb, cols


@pytest.mark.parametrize("data", ["ascii", "binary"])
@pytest.mark.parametrize("colour", ["F", "U", "rgba"])
def test_read_rgb_pcd_fields_in_any_order(tmp_path, data, colour):
    sw = _module()
    rng = np.random.default_rng(11)
    n = 500
    xyz, rgb, cols = _cloud_cols(n, rng, colour)
    cname = "rgba" if colour == "rgba" else "rgb"
    ctype = "F" if colour == "F" else "U"
    spec = [("d8", 8, "F", 1), ("y", 4, "F", 1), ("b1", 1, "U", 1), (cname, 4, ctype, 1), ("x", 4, "F", 1), ("w4", 4, "F", 3), ("s2", 2, "I", 1),
            ("z", 4, "F", 1), ("u8", 8, "U", 2)]
    p = str(tmp_path / "c.pcd")
    _write_pcd(p, spec, cols, n, data)
    gx, gc = sw._read_rgb_pcd(p)
    assert gx.shape == (n, 3) and gx.dtype == np.float32 and gc.dtype == np.uint32
    assert _same(gx, xyz)
    assert np.array_equal(gc, rgb)


def test_read_rgb_pcd_without_points_line_and_signed_colour(tmp_path):
    sw = _module()
    rng = np.random.default_rng(12)
    xyz = rng.uniform(-5, 5, (40, 3)).astype(np.float32)
    rgb = rng.integers(0, 1 << 32, 40, dtype=np.uint64).astype(np.uint32)
    p = str(tmp_path / "c.pcd")
    _write_pcd(p, [("x", 4, "F", 1), ("y", 4, "F", 1), ("z", 4, "F", 1), ("rgba", 4, "I", 1)],
               {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "rgba": rgb.view(np.int32)}, 40, "ascii", header_points=False)
    gx, gc = sw._read_rgb_pcd(p)
    assert _same(gx, xyz) and np.array_equal(gc, rgb)


OBJ = """# a mesh
mtllib m.mtl
o thing
v 0.1 0.2 0.3
v 1e-3 -2.5 3.14159265358979 1.0 0.5 0.25
v   7 8 9
vt 0.5 0.5
vn 0 0 1
v -0.000001 123456.789 1e-40

g group
s off
usemtl mat
f 1 2 3
f 1/1 2/1 3/1 4/1
f 1//1 2//1 4//1
f 4/1/1 3/1/1 2/1/1
v 5.5 6.5 7.5
f -1 -2 -3
f 5 -5 2 3 4
"""


def test_read_obj_forms_and_relative_indices(tmp_path):
    sw = _module()
    p = tmp_path / "m.obj"
    p.write_text(OBJ)
    v, f = sw._read_obj(str(p))
    want = [["0.1", "0.2", "0.3"], ["1e-3", "-2.5", "3.14159265358979"], ["7", "8", "9"], ["-0.000001", "123456.789", "1e-40"], ["5.5", "6.5", "7.5"]]
    exp = np.array([[np.float32(t) for t in r] for r in want], np.float32)
    assert v.dtype == np.float32 and _same(v, exp)
    assert [list(x) for x in f] == [[0, 1, 2], [0, 1, 2, 3], [0, 1, 3], [3, 2, 1], [4, 3, 2], [4, 0, 1, 2, 3]]


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    nv = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    nf = int(next(ln for ln in lines if ln.startswith("element face")).split()[2])
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    vert = np.frombuffer(body[: nv * vt.itemsize], vt)
    faces, o = [], nv * vt.itemsize
    for _ in range(nf):
        c = body[o]
        faces.append(np.frombuffer(body[o + 1: o + 1 + 4 * c], "<i4").tolist())
        o += 1 + 4 * c
    assert o == len(body)
    return head.decode() + "end_header\n", vert, faces


PLY_HEAD = ("ply\nformat binary_little_endian 1.0\ncomment PCL generated\nelement vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {nf}\nproperty list uchar int vertex_indices\nend_header\n")


def test_write_mesh_ply_layout(tmp_path):
    sw = _module()
    rng = np.random.default_rng(13)
    v = rng.normal(size=(300, 3)).astype(np.float32)
    v[7, 1] = np.nan
    c = rng.integers(0, 256, (300, 3)).astype(np.uint8)
    faces = [[int(i) for i in rng.integers(0, 300, rng.integers(1, 9))] for _ in range(200)]
    p = str(tmp_path / "o.ply")
    sw._write_mesh_ply(p, v, c, faces)
    head, vert, fs = _read_ply(p)
    assert head == PLY_HEAD.format(nv=300, nf=200)
    assert _same(np.stack([vert["x"], vert["y"], vert["z"]], 1), v)
    assert np.array_equal(np.stack([vert["r"], vert["g"], vert["b"]], 1), c)
    assert fs == faces


def _good_cloud(path, n=50):
    rng = np.random.default_rng(14)
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    rgb = rng.integers(0, 1 << 24, n).astype(np.uint32)
    _write_pcd(path, [("x", 4, "F", 1), ("y", 4, "F", 1), ("z", 4, "F", 1), ("rgb", 4, "U", 1)],
               {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "rgb": rgb}, n, "binary")


def test_texture_mesh_refusals(tmp_path):
    sw = _module()
    out = tmp_path / "out"
    out.mkdir()
    good_pcd, good_obj = str(tmp_path / "good.pcd"), str(tmp_path / "good.obj")
    _good_cloud(good_pcd)
    (tmp_path / "good.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")

    def pcd(name, text, body=b""):
        p = tmp_path / name
        p.write_bytes(text.encode() + body)
        return str(p)

    hdr = "VERSION 0.7\nFIELDS {f}\nSIZE {s}\nTYPE {t}\nCOUNT {c}\nWIDTH 2\nHEIGHT 1\nPOINTS 2\nDATA {d}\n"
    no_rgb = pcd("norgb.pcd", hdr.format(f="x y z intensity", s="4 4 4 4", t="F F F F", c="1 1 1 1", d="ascii") + "0 0 0 1\n1 1 1 1\n")
    compressed = pcd("comp.pcd", hdr.format(f="x y z rgb", s="4 4 4 4", t="F F F U", c="1 1 1 1", d="binary_compressed"), b"\0" * 64)
    nan_only = pcd("nan.pcd", hdr.format(f="x y z rgb", s="4 4 4 4", t="F F F U", c="1 1 1 1", d="ascii") + "nan 0 0 5\n1 inf 1 7\n")
    short = pcd("short.pcd", hdr.format(f="x y z rgb", s="4 4 4 4", t="F F F U", c="1 1 1 1", d="binary"), b"\0" * 20)
    garbage = pcd("garbage.pcd", "this is not a point cloud\n")
    bad_value = pcd("badval.pcd", hdr.format(f="x y z rgb", s="4 4 4 4", t="F F F U", c="1 1 1 1", d="ascii") + "0 0 zero 5\n1 1 1 7\n")
    xyz8 = pcd("xyz8.pcd", hdr.format(f="x y z rgb", s="8 8 8 4", t="F F F U", c="1 1 1 1", d="ascii") + "0 0 0 5\n1 1 1 7\n")
    (tmp_path / "range.obj").write_text("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    (tmp_path / "range_neg.obj").write_text("v 0 0 0\nf -2 -1 1\n")
    (tmp_path / "badv.obj").write_text("v 0 0\nf 1 1 1\n")
    (tmp_path / "badf.obj").write_text("v 0 0 0\nf 1 x 1\n")
    cases = [
        (good_obj, str(tmp_path / "missing.pcd"), str(out), "cannot read the cloud"),
        (good_obj, garbage, str(out), "no DATA line"),
        (good_obj, short, str(out), "shorter than its header"),
        (good_obj, bad_value, str(out), "bad value"),
        (good_obj, xyz8, str(out), "4-byte floats"),
        (good_obj, compressed, str(out), "binary_compressed"),
        (good_obj, no_rgb, str(out), "no rgb / rgba field"),
        (good_obj, nan_only, str(out), "no finite point"),
        (str(tmp_path / "missing.obj"), good_pcd, str(out), "cannot read the mesh"),
        (str(tmp_path / "range.obj"), good_pcd, str(out), "out of range"),
        (str(tmp_path / "range_neg.obj"), good_pcd, str(out), "out of range"),
        (str(tmp_path / "badv.obj"), good_pcd, str(out), "malformed vertex"),
        (str(tmp_path / "badf.obj"), good_pcd, str(out), "malformed face index"),
        (good_obj, good_pcd, str(tmp_path / "no_such_dir"), "cannot be written"),
        (good_obj, good_pcd, good_pcd, "cannot be written"),
    ]
    for mesh, cloud, dest, why in cases:
        with pytest.raises(ValueError, match=why):
            sw.texture_mesh(mesh, cloud, dest)
        assert not os.path.exists(os.path.join(dest, "texture_mesh.ply"))
    assert os.listdir(out) == []
