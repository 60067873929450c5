// tsdf_mesh_table.h -- the 256-case triangle table of the TSDF mesh (tsdf_mesh.hip), DERIVED at compile time by the rule of
// include/regnet_hip.h "Triangle mesh" (DESIGN.md par. 5); tests/tsdf_mesh_reference.py restates the rule in Python and
// tests/test_tsdf_mesh_reference_cpu.py compares the two through regnet_tsdf_mesh_case.  Integer work only.
//
//   corner c     the cell's low corner voxel plus (c & 1, c >> 1 & 1, c >> 2 & 1); INSIDE when its bit of the case is set.
//   edge (c, a)  joins corner c (bit a clear) to corner c | 1 << a; the twelve are numbered in ascending (c, a).
//   face (k, s)  the corners whose bit k is s, in the cyclic order q0..q3 = (0,0), (1,0), (1,1), (0,1) of their (u, v) bits, u =
//                (k + 1) % 3, v = (k + 2) % 3: counterclockwise seen from +e_k.  Face edge E_i joins q_i to q_(i+1).
//   segments     every maximal run q_i .. q_j of inside corners of a face (not none, not all) is cut off by one segment, which
//                joins E_(i-1) to E_j: two diagonal inside corners are cut off one by one, whatever the rest of the cell holds.
//                Seen from outside the cell it runs clockwise round its run: E_(i-1) -> E_j on a face s = 1, E_j -> E_(i-1) on
//                a face s = 0, so that the right-hand-rule normal of what it bounds points to D > 0.
//   loops        a crossed edge ends one segment and starts one: closed directed loops of 3..7 edges, in ascending order of
//                their lowest edge.
//   fan          loop v_0 .. v_(n-1) from its apex v_0: triangles (v_0, v_i, v_(i+1)), i = 1 .. n - 2.  A diagonal (v_0, v_i), 1 <
//                i < n - 1, both of whose edges lie in one cube face is flat; the apex is the loop's edge with the fewest flat
//                diagonals, the lowest edge number among equals.  (Every loop has an apex with none.)
#pragma once
#include <stdint.h>

namespace tsdf_mesh {

constexpr int CASES = 256, SLOTS = 16, EDGES = 12, MAX_TRIANGLES = 5;

struct Table {
  int8_t edges[CASES][SLOTS];      // three edge numbers per triangle, -1 in the unused slots
  uint8_t triangles[CASES];
  int8_t edge_corner[EDGES], edge_axis[EDGES];
};

constexpr int edge_id(int c, int a) {      // the number of edge (c, a): the edges (c', a') below it
  int e = 0;
  for (int cc = 0; cc < 8; ++cc)
    for (int aa = 0; aa < 3; ++aa) {
      if (cc >> aa & 1) continue;
      if (cc == c && aa == a) return e;
      ++e;
    }
  return -1;
}

constexpr int edge_between(int c0, int c1) {
  const int lo = c0 < c1 ? c0 : c1, d = c0 ^ c1;
  return edge_id(lo, d == 1 ? 0 : d == 2 ? 1 : 2);
}

constexpr int face_corner(int k, int s, int i) {
  const int u = (k + 1) % 3, v = (k + 2) % 3;
  const int qu = (i == 1 || i == 2) ? 1 : 0, qv = i >> 1;
  return s << k | qu << u | qv << v;
}

constexpr bool same_face(int c0, int a0, int c1, int a1) {
  for (int k = 0; k < 3; ++k)
    if (k != a0 && k != a1 && (c0 >> k & 1) == (c1 >> k & 1)) return true;
  return false;
}

constexpr Table make_table() {
  Table t = {};
  for (int c = 0, e = 0; c < 8; ++c)
    for (int a = 0; a < 3; ++a)
      if (!(c >> a & 1)) { t.edge_corner[e] = (int8_t)c; t.edge_axis[e] = (int8_t)a; ++e; }
  int face_edge[6][4] = {}, face_q[6][4] = {};
  for (int f = 0; f < 6; ++f)
    for (int i = 0; i < 4; ++i) {
      face_q[f][i] = face_corner(f >> 1, f & 1, i);
      face_edge[f][i] = edge_between(face_corner(f >> 1, f & 1, i), face_corner(f >> 1, f & 1, (i + 1) & 3));
    }
  for (int cs = 0; cs < CASES; ++cs) {
    for (int i = 0; i < SLOTS; ++i) t.edges[cs][i] = -1;
    int next[EDGES] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    for (int f = 0; f < 6; ++f) {      // face (k, s) = (f >> 1, f & 1)
      const int* E = face_edge[f];
      int in[4] = {0, 0, 0, 0}, n_in = 0;
      for (int i = 0; i < 4; ++i) {
        in[i] = cs >> face_q[f][i] & 1;
        n_in += in[i];
      }
      if (n_in == 0 || n_in == 4) continue;
      for (int i = 0; i < 4; ++i) {
        if (!in[i] || in[(i + 3) & 3]) continue;      // a run starts at q_i
        int j = i;
        while (in[(j + 1) & 3]) j = (j + 1) & 3;
        const int first = E[(i + 3) & 3], last = E[j];
        if (f & 1) next[first] = last; else next[last] = first;
      }
    }
    bool seen[EDGES] = {};
    int slot = 0;
    for (int e = 0; e < EDGES; ++e) {
      if (next[e] < 0 || seen[e]) continue;
      int loop[8] = {}, n = 0;
      for (int v = e; !seen[v]; v = next[v]) { seen[v] = true; loop[n++] = v; }
      int best = 0, best_flat = 99;
      for (int j = 0; j < n; ++j) {
        int flat = 0;
        for (int i = 2; i < n - 1; ++i) {
          const int a = loop[j], b = loop[(j + i) % n];
          flat += same_face(t.edge_corner[a], t.edge_axis[a], t.edge_corner[b], t.edge_axis[b]) ? 1 : 0;
        }
        if (flat < best_flat || (flat == best_flat && loop[j] < loop[best])) { best = j; best_flat = flat; }
      }
      for (int i = 1; i < n - 1; ++i) {
        t.edges[cs][slot++] = (int8_t)loop[best];
        t.edges[cs][slot++] = (int8_t)loop[(best + i) % n];
        t.edges[cs][slot++] = (int8_t)loop[(best + i + 1) % n];
      }
    }
    t.triangles[cs] = (uint8_t)(slot / 3);
  }
  return t;
}

}  // namespace tsdf_mesh
