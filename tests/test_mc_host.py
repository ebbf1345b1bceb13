"""Host tests of the surface reconstruction (no GPU): the marching-cubes case tables of csrc/mvr_mc_tables.h, read through
mvr_mc_case (rule M10 in include/mvr_hip.h) -- written out from memory, so proved here row by row and all 256 together --, the
numpy restatement tests/mc_ref.py on lattices with known answers, and the mesh PLY reader and writer of include/mvr/io.hpp
through tests/cxx/mc_driver.cpp (compiled here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

import mc_ref as R
from mc_cases import read_ply

F32 = np.float32


# ------------------------------------------------------------------ the tables

def test_every_row_of_the_tables(mvr):
    edge, tri = R.tables()
    assert edge.shape == (256,) and tri.shape == (256, 16)
    for cube in range(256):
        row = tri[cube]
        n = int(np.argmax(row < 0))
        assert row[15] == -1 and (row[n:] == -1).all() and (row[:n] >= 0).all() and (row[:n] < 12).all(), cube
        assert n % 3 == 0 and n <= 15, cube
        used = set(int(e) for e in row[:n])
        bits = set(e for e in range(12) if edge[cube] >> e & 1)
        crossed = set(e for e in range(12) if (cube >> R.EDGE_A[e] & 1) != (cube >> R.EDGE_B[e] & 1))
        assert used == bits == crossed, cube
        for k in range(0, n, 3):      # no triangle names an edge twice
            assert len(set(row[k:k + 3])) == 3, cube
    assert edge[0] == 0 and edge[255] == 0 and (edge[np.arange(256)] == edge[255 - np.arange(256)]).all()


def test_mc_case_refuses_what_is_no_row(mvr):
    e, t = C.c_uint16(7), (C.c_int8 * 16)(*([7] * 16))
    for cube in (-1, 256, 1 << 20):
        assert mvr._lib.mvr_mc_case(cube, C.byref(e), t) == mvr.E_ARG and e.value == 7 and list(t) == [7] * 16
    assert mvr._lib.mvr_mc_case(5, None, None) == mvr.OK


def test_library_exports_the_entries(mvr):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    for sym in ("mvr_cloud_marching_cubes_hoppe", "mvr_mc_default_params", "mvr_mc_case"):
        assert sym in mvr.SIGNATURES and re.search(r" T %s$" % sym, r.stdout, re.M), sym
    assert C.sizeof(mvr.McParams) == 32
    assert [f[0] for f in mvr.McParams._fields_] == ["res", "iso_level", "percentage_extend_grid", "dist_ignore", "weld", "fma_dist"]
    p = mvr.McParams((C.c_int * 3)(9, 9, 9), 9.0, 9.0, 9.0, 9, 9)
    mvr._lib.mvr_mc_default_params(C.byref(p))
    assert (list(p.res), p.iso_level, p.percentage_extend_grid, p.dist_ignore, p.weld, p.fma_dist) == ([32, 32, 32], 0.0, 0.0, -1.0, 0, 0)
    hdr = open(os.path.join(ROOT, "include", "mvr_hip.h")).read()
    for m in range(1, 16):
        assert re.search(r"^ \* {1,2}M%d\. " % m, hdr[hdr.index("pcl::MarchingCubesHoppe"):], re.M), m
    assert "PARITY WITH PCL UNPINNED" in hdr and re.search(r"#define MVR_MC_MAX_VERTICES \(1ull << 27\)", hdr) and mvr.MC_MAX_VERTICES == 1 << 27
    assert hasattr(mvr.Context, "marching_cubes_hoppe")
    # the tables stand once: no other source file carries a row of them
    row = "{2, 8, 3, 2, 10, 8, 10, 9, 8,"
    hits = [f for dp, _, fs in os.walk(ROOT) if "/build" not in dp and "/.git" not in dp for f in fs
            if f.endswith((".h", ".hip", ".hpp", ".cpp", ".c", ".py")) and f != "test_mc_host.py" and row in open(os.path.join(dp, f), errors="ignore").read()]
    assert hits == ["mvr_mc_tables.h"]


# ------------------------------------------------------------------ closed meshes

def mesh_of(values, lower=(0.0, 0.0, 0.0), size=(1.0, 1.0, 1.0), iso=0.0):
    m = R.march(np.asarray(values, F32), F32(lower), F32(size), iso)
    v, i = R.weld(m["soup"], m["edge_key"])
    return m, v, i


def test_random_sign_lattices_give_closed_oriented_meshes(mvr):
    """values of +-1 on the unit lattice: every mu is exactly 0.5 and every vertex an exact half-integer; one layer of +1 around
    it closes the surface.  Welded by edge key, every directed edge occurs once and its reverse once -- which no table with a
    wrong row, a row for the wrong cube or an inconsistent choice on an ambiguous face survives -- and the three lattices
    together meet all 256 cubes."""
    seen = set()
    for seed in (0, 1, 2):
        rng = np.random.default_rng(seed)
        val = np.ones((12, 12, 12), F32)
        val[1:-1, 1:-1, 1:-1] = rng.choice(F32([-1.0, 1.0]), (10, 10, 10))
        m, v, i = mesh_of(val)
        assert not m["skipped"].any() and len(m["soup"]) % 3 == 0 and len(i) == len(m["soup"]) > 3000
        assert np.array_equal(m["soup"] * 2, np.round(m["soup"] * 2)) and ((m["soup"] * 2) % 2 == 1).sum(1).tolist() == [1] * len(m["soup"])
        assert R.closed_and_oriented(i), seed
        # a welded vertex IS its edge: the same key, the same position, whichever cell computed it
        first = {}
        for key, pos in zip(m["edge_key"].tolist(), map(tuple, m["soup"].tolist())):
            assert first.setdefault(key, pos) == pos
        assert len(first) == len(v)
        seen |= set(int(c) for c in m["cube"])
    assert seen == set(range(256))


def test_sphere_distance_field(mvr):
    """the analytic field |x| - r on a lattice of spacing h: a closed, consistently oriented surface of Euler characteristic 2.
    Volume: a mesh vertex p on a lattice edge is a zero of the LINEAR interpolant of f along that edge; f restricted to a line has
    |f''| <= 1 / |x|, so the interpolant is off by at most h^2 / (8 (r - sqrt(3) h)) =: d1 there, and f(p) is the distance of p from
    the sphere: every vertex lies within d1 of it.  A triangle lies inside one cell (diameter sqrt(3) h), never outside the convex
    ball of radius r + d1, and dips below its corners by at most the sagitta (sqrt(3) h)^2 / (4 (r - d1)) (twice the small-angle
    value, to be safe).  The mesh therefore lies in the shell [r - d1 - 3 h^2 / (4 (r - d1)), r + d1] and, being one closed
    surface around the centre, encloses a volume between the two balls'.  The signed volume is POSITIVE: with values negative
    inside, the tables wind a triangle counter-clockwise seen from the positive side -- the documented orientation (outward for
    normals that point out of the object)."""
    h, r, res = 0.125, 0.8, 17
    ax = (-1.0 + h * np.arange(res)).astype(F32)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    val = (np.sqrt(X.astype(np.float64) ** 2 + Y.astype(np.float64) ** 2 + Z.astype(np.float64) ** 2) - r).astype(F32)
    m, v, i = mesh_of(val, (-1.0, -1.0, -1.0), (h, h, h))
    assert R.closed_and_oriented(i) and R.euler(len(v), i) == 2
    d1 = h * h / (8.0 * (r - np.sqrt(3.0) * h))
    inner, outer = r - d1 - 3.0 * h * h / (4.0 * (r - d1)), r + d1
    radius = np.linalg.norm(v.astype(np.float64), axis=1)
    assert (np.abs(radius - r) <= d1 + 1e-6).all()
    vol = R.signed_volume(v, i)
    assert 4.0 / 3.0 * np.pi * inner ** 3 <= vol <= 4.0 / 3.0 * np.pi * outer ** 3
    # the other sign of the field turns every triangle round
    m2, v2, i2 = mesh_of(-val, (-1.0, -1.0, -1.0), (h, h, h))
    assert R.closed_and_oriented(i2) and np.isclose(R.signed_volume(v2, i2), -vol, rtol=1e-6)


def test_reference_rules_on_small_inputs(mvr):
    # M2-M4: the box of the finite points, widened, divided by res (not res - 1)
    p = F32([[0, 0, 0], [4, 8, 2], [np.nan, 100, 100], [1, np.inf, 1]])
    lower, size = R.box(p, (4, 4, 2), 0.5)
    assert lower.tolist() == [-1.0, -2.0, -0.5] and size.tolist() == [1.5, 3.0, 1.5]
    assert R.lattice(lower, size, (4, 4, 2))[3, 3, 1].tolist() == [3.5, 7.0, 1.0]      # one voxel short of upper = (5, 10, 2.5)
    assert R.box(p[2:], (2, 2, 2), 0.0) is None
    # M5: ties to the lowest index, the non-finite point nobody's neighbour, the SQUARED distance against dist_ignore
    q = F32([[1.2, 0, 0], [-1.2, 0, 0], [np.nan, 0, 0], [1.2, 0, 0]])
    idx, d2 = R.nearest(F32([[0, 0, 0], [0.9, 0, 0]]), q)
    assert idx.tolist() == [0, 0] and d2[0] == F32(1.2) * F32(1.2)
    n = F32([[1, 0, 0]] * 4)
    lattice_x = [-1.2, 0.0]                                     # res 2: the second vertex is the middle of the box
    g = R.values(q, n, (2, 2, 2), dist_ignore=1.3)[0]           # the middle vertex: distance 1.2 < 1.3, but d2 = 1.44 is not
    assert g[0, 0, 0] == 0.0 and np.isnan(g[1, 0, 0]) and R.values(q, n, (2, 2, 2))[1][0] == F32(lattice_x[0])
    assert R.values(q, n, (2, 2, 2), dist_ignore=1.5)[0][1, 0, 0] == -F32(1.2)
    # a cell with a NaN corner emits nothing; M13 numbers the vertices in order of first use
    val = np.ones((3, 2, 2), F32)
    val[0, 0, 0] = -1
    val[2, 1, 1] = np.nan
    m, v, i = mesh_of(val)
    assert m["skipped"].tolist() == [False, True] and len(m["soup"]) == 3 and i.tolist() == [0, 1, 2]
    assert sorted(m["edge_key"].tolist()) == [0, 1, 2]           # the three edges at vertex 0, axes x, y, z


# ------------------------------------------------------------------ mesh PLY

@pytest.fixture(scope="module")
def driver(built, tmp_path_factory):
    built.build_hip()
    exe = str(tmp_path_factory.mktemp("mc_host") / "mc_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "mc_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_mesh_ply_round_trip(driver, tmp_path):
    rng = np.random.default_rng(4)
    v = (rng.standard_normal((40, 3)) * [1e-3, 1.0, 1e5]).astype(F32)
    faces = [rng.choice(40, k, replace=False).tolist() for k in [3] * 20 + [4, 5, 3]]
    for name, vv, ff in (("mesh", v, faces), ("no_faces", v[:7], []), ("nothing", v[:0], [])):
        src, dst = tmp_path / (name + ".ply"), tmp_path / (name + "_out.ply")
        with open(src, "w") as f:
            f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(vv))
            f.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(ff))
            f.writelines("%.9g %.9g %.9g\n" % tuple(float(c) for c in p) for p in vv)
            f.writelines("%d %s\n" % (len(p), " ".join(map(str, p))) for p in ff)
        r = run(driver, "roundtrip", src, dst)
        assert r.returncode == 0 and r.stdout.split() == [str(len(vv)), str(len(ff))], (r.stdout, r.stderr)
        got_v, got_f = read_ply(dst)
        assert R.same_bits(got_v, vv) and got_f == ff
        head = open(dst).read().split("end_header")[0]
        assert "element vertex %d\n" % len(vv) in head and "element face %d\nproperty list uchar int vertex_indices\n" % len(ff) in head


def test_foreign_and_broken_mesh_files(driver, tmp_path):
    foreign = tmp_path / "foreign.ply"
    foreign.write_text("ply\r\nformat ascii 1.0\r\ncomment made by hand\r\nobj_info nothing\r\n"
                       "element vertex 4\nproperty double x\nproperty float y\nproperty uchar red\nproperty float z\n"
                       "element edge 2\nproperty int vertex1\nproperty int vertex2\n"
                       "element face 2\nproperty uchar flags\nproperty list uchar float texcoord\nproperty list uint uint vertex_index\n"
                       "element material 1\nproperty float shine\nend_header\n"
                       "0 0 200 0\n1 0 9 0\n0 1 10 0.5\n1 1 7 -2.5\n0 1\n2 3\n"
                       "5 2 0.5 0.25 3 0 1 2\n6 0 4 3 2 1 0\n0.75\n")
    out = tmp_path / "foreign_out.ply"
    r = run(driver, "roundtrip", foreign, out)
    assert r.returncode == 0 and r.stdout.split() == ["4", "2"], (r.stdout, r.stderr)
    v, f = read_ply(out)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0.5], [1, 1, -2.5]] and f == [[0, 1, 2], [3, 2, 1, 0]]
    good = "ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n"
    broken = {"binary": good.replace("ascii", "binary_little_endian"), "index": good.replace("3 0 1 2", "3 0 1 3"),
              "short_face": good.replace("3 0 1 2", "3 0 1"), "truncated": good[:good.index("0 1 0\n")], "no_z": good.replace("property float z\n", ""),
              "negative": good.replace("3 0 1 2", "3 0 -1 2"), "not_ply": good.replace("ply\n", "plx\n", 1)}
    for name, text in broken.items():
        p = tmp_path / (name + ".ply")
        p.write_text(text)
        r = run(driver, "roundtrip", p, tmp_path / "never.ply")
        assert r.returncode == 4, (name, r.stdout, r.stderr)
    assert not (tmp_path / "never.ply").exists()
    p = tmp_path / "good.ply"
    p.write_text(good)
    assert run(driver, "roundtrip", p, tmp_path / "good_out.ply").stdout.split() == ["3", "1"]
