"""tests/tsdf_mesh_reference.py -- the generator of the marching-cubes table and the plain-loop mesh of a TSDF volume -- held to
things it can be wrong about, and the table compiled into the library (csrc/tsdf_mesh_table.h, read through
``regnet_tsdf_mesh_case``) held to the generator.  No GPU: the library is loaded for the host-only accessor alone.

The per-case properties are computed HERE from the case's bits, not taken from the generator's helpers: which edges are crossed,
which segments a face's four signs ask for, where the outside is.
"""
import collections
import ctypes

import numpy as np
import pytest

from . import tsdf_mesh_reference as mref
from . import tsdf_reference as ref
from .icp_projective_reference import look_at, rectangle, render, sphere

f32 = np.float32
W, H = 64, 48
K = (400.0, 400.0, 31.5, 23.5)
SMALL = dict(voxel=0.002, trunc=0.01, origin=(-0.02, -0.02, 0.38), dims=(20, 20, 20), max_points=4096)
CORNER_XYZ = np.array([(c & 1, c >> 1 & 1, c >> 2 & 1) for c in range(8)], dtype=np.float64)
EDGE_ENDS = [(c, c | 1 << a) for c in range(8) for a in range(3) if not c >> a & 1]        # ascending (c, a)
EDGE_MID = np.array([(CORNER_XYZ[a] + CORNER_XYZ[b]) / 2 for a, b in EDGE_ENDS])


def _case_triangles(table, case):
    row = [int(e) for e in table[case]]
    used = [e for e in row if e >= 0]
    assert len(used) % 3 == 0 and row[len(used):] == [-1] * (16 - len(used))
    return [tuple(used[i:i + 3]) for i in range(0, len(used), 3)]


def _crossed(case):
    return {e for e, (a, b) in enumerate(EDGE_ENDS) if (case >> a & 1) != (case >> b & 1)}


def _face_of(e0, e1):
    """The cube faces (axis, side) that hold both edges."""
    out = []
    for k in range(3):
        for s in range(2):
            if all(CORNER_XYZ[c][k] == s for e in (e0, e1) for c in EDGE_ENDS[e]):
                out.append((k, s))
    return out


def _expected_segments(case, k, s):
    """What the face's own four signs ask for, as undirected edge pairs: two crossed edges are joined; with four, every inside
    corner is cut off: its two face edges are joined."""
    corners = [c for c in range(8) if CORNER_XYZ[c][k] == s]
    edges = [e for e, (a, b) in enumerate(EDGE_ENDS) if a in corners and b in corners]
    crossed = [e for e in edges if e in _crossed(case)]
    if len(crossed) == 2:
        return {frozenset(crossed)}
    if len(crossed) == 4:
        return {frozenset(e for e in edges if c in EDGE_ENDS[e]) for c in corners if case >> c & 1}
    assert not crossed
    return set()


def test_the_generator_matches_the_figures_of_its_rule():
    """820 triangles over the 256 cases, 5 at most per case, 7 edges in the longest loop; with the apex at a loop's lowest edge 34
    fan diagonals lie inside a cube face, with the preferred apex none."""
    assert mref.TABLE.shape == (256, 16) and mref.TABLE.dtype == np.int8
    assert int(mref.TRIANGLES.sum()) == 820 and int(mref.TRIANGLES.max()) == 5
    assert max(len(loop) for case in range(256) for loop in mref.case_loops(case)) == 7
    assert sum(mref.flat_diagonals(loop) for case in range(256) for loop in mref.case_loops(case, False)) == 34
    assert sum(mref.flat_diagonals(loop) for case in range(256) for loop in mref.case_loops(case)) == 0


def test_the_compiled_table_is_the_generators():
    from regnet_for_3d_grasping_amd import _lib
    buf = (ctypes.c_int8 * 16)()
    for case in range(256):
        assert _lib.lib.regnet_tsdf_mesh_case(case, buf) == 0
        assert list(buf) == mref.TABLE[case].tolist(), case
    for case in (-1, 256, 1 << 40):
        assert _lib.lib.regnet_tsdf_mesh_case(case, buf) == -1, case            # REGNET_ERR_SHAPE
    assert _lib.lib.regnet_tsdf_mesh_case(3, None) == -2                          # REGNET_ERR_NULL
    assert _lib.lib.regnet_tsdf_mesh_blocks(3, 3, 29) == 2 and _lib.lib.regnet_tsdf_mesh_blocks(0, 3, 3) == -1
    assert _lib.lib.regnet_tsdf_mesh_scratch_bytes(2, 3, 4) == 96 and _lib.lib.regnet_tsdf_mesh_scratch_bytes(1 << 14, 1 << 14, 2) == -1


@pytest.mark.parametrize("case", range(256))
def test_table_properties(case):
    tris = _case_triangles(mref.TABLE, case)
    assert len(tris) <= 5
    if case in (0, 255):
        assert tris == []
    # the triangle edges are exactly the crossed edges, and the complement crosses the same ones
    assert {e for t in tris for e in t} == _crossed(case) == {e for t in _case_triangles(mref.TABLE, 255 - case) for e in t}
    # the triangle sides lying in a face are exactly the segments that face's signs ask for
    in_face = collections.defaultdict(set)
    sides = collections.Counter()
    for a, b, c in tris:
        assert len({a, b, c}) == 3
        for x, y in ((a, b), (b, c), (c, a)):
            sides[(x, y)] += 1
            for face in _face_of(x, y):
                in_face[face].add(frozenset((x, y)))
    for k in range(3):
        for s in range(2):
            assert in_face[(k, s)] == _expected_segments(case, k, s), (k, s)
    # inside the cell the triangles join up: a side that is not a face segment is used once in each direction, a segment once
    for (x, y), n in sides.items():
        assert n == 1
        assert ((y, x) in sides) != any(frozenset((x, y)) in v for v in in_face.values())
    # every triangle's right-hand-rule normal points from the inside corners of its edges to the outside ones
    for tri in tris:
        p = EDGE_MID[list(tri)]
        normal = np.cross(p[1] - p[0], p[2] - p[0])
        ends = {c for e in tri for c in EDGE_ENDS[e]}
        inside = [c for c in ends if case >> c & 1]
        outside = [c for c in ends if not case >> c & 1]
        assert np.linalg.norm(normal) > 0
        assert normal @ (CORNER_XYZ[outside].mean(axis=0) - CORNER_XYZ[inside].mean(axis=0)) > 0


def _edge_use(tri):
    use = collections.Counter()
    for a, b, c in tri:
        for x, y in ((a, b), (b, c), (c, a)):
            use[(int(x), int(y))] += 1
    return use


def _closed(tri):
    """Every undirected edge is used by exactly two triangles, once in each direction."""
    use = _edge_use(tri)
    return all(n == 1 for n in use.values()) and all((y, x) in use for x, y in use)


def test_random_sign_field_is_a_closed_orientable_surface():
    rng = np.random.RandomState(12)
    inside = rng.uniform(size=(12, 12, 12)) < 0.5
    inside[0] = inside[-1] = inside[:, 0] = inside[:, -1] = inside[:, :, 0] = inside[:, :, -1] = False
    tri = mref.sign_field_mesh(inside)
    assert len(tri) > 1000 and _closed(tri)
    # per connected component V - E + F = 2 - 2 g with an integer g >= 0
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in tri.tolist():
        parent[find(a)] = find(b)
        parent[find(b)] = find(c)
    V, E, F = collections.Counter(), collections.Counter(), collections.Counter()
    for v in parent:
        V[find(v)] += 1
    for (x, y) in _edge_use(tri):
        if x < y:
            E[find(x)] += 1
    for a, _, _ in tri.tolist():
        F[find(a)] += 1
    assert len(V) > 3
    for root in V:
        chi = V[root] - E[root] + F[root]
        assert chi <= 2 and chi % 2 == 0, (root, chi)


def _geometry(out):
    """-> per triangle (twice its area vector, the mean of its three vertex normals), float64, of a ``mref.mesh`` result without
    dropped triangles."""
    kt = int(out["num"][0])
    tri = out["tri"][:kt]
    assert (tri >= 0).all() and out["num"][2] == 0 and out["num"][3] == 0
    p = out["surface"]["xyz"].astype(np.float64)[tri]
    n = out["surface"]["normal"].astype(np.float64)[tri].mean(axis=1)
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), n, p


def test_sphere_from_two_views_faces_outwards_and_is_open():
    """The two views of tests/test_tsdf_reference_cpu.py see the near cap of the sphere, so the mesh is open (its border is where
    a corner was not observed) and no volume is held; every triangle faces where its vertices' normals face."""
    c, radius = np.array([0.0, 0.0, 0.43]), 0.04
    poses = [look_at((0.0, 0.0, 0.0), c, up=(0.0, -1.0, 0.0)), look_at((0.25, 0.0, 0.08), c, up=(0.0, -1.0, 0.0))]
    clouds = [(render([sphere(c, radius)], W, H, K, pose), None) for pose in poses]
    vol, _, surface = ref.fuse_volume(clouds, [(W, H, K)] * 2, poses, **SMALL)
    out = mref.mesh(vol, 8192, surface)
    area2, normal, _ = _geometry(out)
    assert len(area2) > 300
    assert ((area2 * normal).sum(axis=1) > 0).all()
    use = _edge_use(out["tri"][:len(area2)])
    assert all(n == 1 for n in use.values()) and not all((y, x) in use for x, y in use)      # oriented, with a border


def test_fronto_parallel_plane_faces_the_camera_and_has_its_area():
    """The plane of tests/test_tsdf_reference_cpu.py at z0 = 0.4137 m: 19 x 19 cells in x, y are crossed, two triangles each.  Over
    the window between the voxel centres 3 and 16 in x and in y the mesh is a tiling of a (13 voxel)^2 square: a triangle of a
    cell lies wholly inside or outside it.  The bound: a centre carries two roundings and the spacing of two centres is off the
    voxel by at most 4 eps |x| / voxel = 2.4e-6 relative over one voxel, 13 times less over the window; float32(0.002) is off
    0.002 by 2^-25 relative; z is within 3e-7 m of z0 (that test's bound), a tilt of at most 6e-7 m per 2 mm, which lengthens an
    area by less than its square, 1e-7.  In all below 1e-6 relative."""
    z0 = 0.4137
    xyz = render([rectangle((-1.0, -1.0, z0), (2.0, 0, 0), (0, 2.0, 0))], W, H, K)
    vol = ref.Volume(**SMALL)
    vol.integrate(xyz, None, W, H, K)
    out = mref.mesh(vol, 4096)
    area2, normal, p = _geometry(out)
    assert len(area2) == 2 * 19 * 19
    assert ((area2 * normal).sum(axis=1) > 0).all() and (area2[:, 2] < 0).all()               # towards the camera at the origin
    assert _edge_use(out["tri"][:len(area2)]) and not _closed(out["tri"][:len(area2)])
    centres = vol.centres().astype(np.float64)
    lo, hi = centres[3 + 20 * 3][:2], centres[16 + 20 * 16][:2]
    centroid = p.mean(axis=1)
    window = ((centroid[:, :2] > lo) & (centroid[:, :2] < hi)).all(axis=1)
    assert window.sum() == 2 * 13 * 13
    area = 0.5 * np.linalg.norm(area2[window], axis=1).sum()
    exact = (13 * 0.002) ** 2
    print("plane: window area %.12g m^2 against %.12g" % (area, exact))
    assert abs(area - exact) <= 1e-6 * exact


def test_an_unobserved_voxel_removes_exactly_the_cells_that_touch_it():
    z0 = 0.4137
    xyz = render([rectangle((-1.0, -1.0, z0), (2.0, 0, 0), (0, 2.0, 0))], W, H, K)
    vol = ref.Volume(**SMALL)
    vol.integrate(xyz, None, W, H, K)
    whole = mref.mesh(vol, 4096)
    iz = int(np.floor((z0 - 0.38) / 0.002 - 0.5))            # the layer under the crossing
    assert vol.D[(iz * 20 + 9) * 20 + 7] > 0 > vol.D[((iz + 1) * 20 + 9) * 20 + 7]
    v = (iz * 20 + 9) * 20 + 7
    vol.W[v] = 0
    holed = mref.mesh(vol, 4096)
    touching = {v - dx - 20 * dy - 400 * dz for dx, dy, dz in mref.CORNERS}
    before, after = collections.Counter(whole["cells"].tolist()), collections.Counter(holed["cells"].tolist())
    gone = {cell: n for cell, n in before.items() if cell in touching}
    assert len(gone) == 4 and all(cell not in after for cell in touching)                     # (the four cells of its layer)
    assert after == collections.Counter({cell: n for cell, n in before.items() if cell not in touching})
    assert holed["num"][1] == whole["num"][1] - sum(gone.values()) and holed["num"][2] == 0


def test_a_zero_distance_gives_zero_area_triangles_and_a_closed_mesh():
    """Voxels (2..3)^3 of 5^3 are inside but for (2,2,2), which holds D = 0 -- outside: the three edges from it to its upper
    neighbours cross with s = 0, so their three vertices all lie on its centre, and the one triangle of the cell at (2,2,2) --
    seven corners inside -- has no area; so have those of the neighbouring cells with two of the three.  They are kept: every
    edge of the mesh still has its two triangles."""
    D = np.full((5, 5, 5), 0.5, dtype=np.float32)            # [iz, iy, ix]
    D[2:4, 2:4, 2:4] = -0.5
    D[2, 2, 2] = 0.0
    vol = ref.Volume(voxel=0.5, trunc=1.0, origin=(0.0, 0.0, 0.0), dims=(5, 5, 5), max_points=256)
    vol.D, vol.W = D.reshape(-1).copy(), np.full((125,), 1, dtype=np.int32)
    out = mref.mesh(vol, 256)
    area2, _, p = _geometry(out)
    assert _closed(out["tri"][:len(area2)])
    flat = np.linalg.norm(area2, axis=1) == 0
    assert flat.sum() >= 1 and (~flat).sum() > 8
    centre = vol.centres()[(2 * 5 + 2) * 5 + 2].astype(np.float64)
    assert any((p[i] == centre).all() for i in np.nonzero(flat)[0])                           # all three vertices on the voxel centre
    # ... and -0.0 is outside as well: the same triangles
    vol.D[(2 * 5 + 2) * 5 + 2] = f32(-0.0)
    assert np.array_equal(mref.mesh(vol, 256)["tri"], out["tri"])


def test_capacity_and_dropped_triangles_in_the_restatement():
    """``max_triangles`` below the total keeps the triangles of the smallest cells; ``max_points`` below the surface's rows
    writes (-1, -1, -1) in place of every triangle that lost a vertex."""
    rng = np.random.RandomState(3)
    vol = ref.Volume(voxel=0.5, trunc=1.0, origin=(0.0, 0.0, 0.0), dims=(6, 5, 4), max_points=1024)
    vol.D, vol.W = rng.uniform(-1, 0.99, size=120).astype(np.float32), np.ones((120,), dtype=np.int32)
    full = mref.mesh(vol, 1024)
    total = int(full["num"][1])
    assert full["num"].tolist() == [total, total, 0, 0] and total > 50 and (np.diff(full["cells"]) >= 0).all()
    few = mref.mesh(vol, 40)
    assert few["num"].tolist() == [40, total, 0, 1] and np.array_equal(few["tri"], full["tri"][:40])
    vol.p["max_points"] = int(full["surface"]["num"][0]) // 2
    cut = mref.mesh(vol, 1024)
    lost = (full["tri"][:total] >= vol.p["max_points"]).any(axis=1)
    assert 0 < lost.sum() < total and cut["num"].tolist() == [total, total, int(lost.sum()), 0]
    assert (cut["tri"][:total][lost] == -1).all() and np.array_equal(cut["tri"][:total][~lost], full["tri"][:total][~lost])
