// Stand-alone run of the mesh-distance twin (meshsdf_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_meshsdf.h), so a vertex gathered through an index that is out of range, or an output written past n_pts, is an error
// report and a non-zero exit.  It covers the edge cases of the rules: degenerate triangles and out-of-range indices among valid ones,
// non-finite vertices and points, n_faces = 0, a mesh without a valid face, null optional outputs and slice counts beyond the face count.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "meshsdf_host.cpp"

static int fail(const char* what) {
  fprintf(stderr, "meshsdf_host_main: %s\n", what);
  return 1;
}

int main() {
  // the cube [-1, 1]^3, 12 triangles, then the troublemakers
  std::vector<float> verts = {-1, -1, -1, 1, -1, -1, 1, 1, -1, -1, 1, -1, -1, -1, 1, 1, -1, 1, 1, 1, 1, -1, 1, 1};
  std::vector<int32_t> cube = {0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 3, 7, 6, 3, 6, 2, 0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5};
  const int n_cube_verts = 8;
  verts.insert(verts.end(), {NAN, 0.f, 0.f, INFINITY, 1.f, 2.f});  // vertices 8 and 9
  const int n_verts = 10;
  std::vector<int32_t> faces;
  const int32_t bad[][3] = {{0, 0, 1}, {0, 1, 1}, {2, 2, 2}, {0, 1, 10}, {-1, 2, 3}, {0, 1, 8}, {9, 1, 2}, {2147483647, 0, 1}, {0, 6, 6}};
  for (int f = 0; f < 12; ++f) {
    faces.insert(faces.end(), bad[f % 9], bad[f % 9] + 3);
    faces.insert(faces.end(), cube.begin() + 3 * f, cube.begin() + 3 * f + 3);
  }
  const int n_faces = (int)faces.size() / 3;  // 24: the odd ones are the cube
  std::vector<float> pts = {0.f, 0.f, 0.f, 0.25f, -0.5f, 0.125f, 3.f, 0.f, 0.f, 2.f, 2.f, 2.f, 1.f, 1.f, 1.f, NAN, 0.f, 0.f, 0.f, INFINITY, 0.f, 0.f, 0.f, -INFINITY,
                            1.5f, 1.5f, 0.f};
  const long n_pts = (long)pts.size() / 3;
  const float want[] = {-1.f, -0.5f, 2.f, 1.7320508f, 0.f, NAN, NAN, NAN, 0.70710678f};
  std::vector<float> sdf(n_pts), d2(n_pts), wsum(n_pts), closest(3 * n_pts), sdf_s(n_pts), closest_s(3 * n_pts), sdf_c(n_pts);
  std::vector<int32_t> face(n_pts), face_s(n_pts);
  std::vector<uint8_t> valid(n_faces);
  meshsdf_host_valid(verts.data(), faces.data(), n_verts, n_faces, valid.data());
  for (int f = 0; f < n_faces; ++f)
    if (valid[f] != (f & 1)) return fail("validity");
  meshsdf_host_query(verts.data(), faces.data(), n_verts, n_faces, pts.data(), n_pts, sdf.data(), d2.data(), wsum.data(), face.data(), closest.data());
  // the cube alone gives the same distances, and faces f / 2
  std::vector<int32_t> face_c(n_pts);
  meshsdf_host_query(verts.data(), cube.data(), n_cube_verts, 12, pts.data(), n_pts, sdf_c.data(), nullptr, nullptr, face_c.data(), nullptr);
  for (long i = 0; i < n_pts; ++i) {
    const bool nan_pt = want[i] != want[i];
    if (nan_pt) {
      if (sdf[i] == sdf[i] || face[i] != -1) return fail("a non-finite point must give NaN and face -1");
      continue;
    }
    if (fabsf(sdf[i] - want[i]) > 1e-6f) return fail("cube distance");
    if (sdf[i] != sdf_c[i] || face[i] != 2 * face_c[i] + 1) return fail("invalid faces changed the result");
  }
  const int slices[] = {1, 2, 3, 7, n_faces + 5};
  for (int n : slices) {
    meshsdf_host_query_sliced(verts.data(), faces.data(), n_verts, n_faces, pts.data(), n_pts, n, sdf_s.data(), nullptr, nullptr, face_s.data(), closest_s.data());
    for (long i = 0; i < n_pts; ++i) {
      if (face_s[i] != face[i]) return fail("sliced face");
      if (sdf[i] == sdf[i] && fabsf(sdf_s[i]) != fabsf(sdf[i])) return fail("sliced distance");
      for (int a = 0; a < 3; ++a)
        if (closest[3 * i + a] == closest[3 * i + a] && closest_s[3 * i + a] != closest[3 * i + a]) return fail("sliced closest point");
    }
  }
  // no faces at all (null mesh pointers), and a mesh without a valid face
  meshsdf_host_query(nullptr, nullptr, 0, 0, pts.data(), n_pts, sdf.data(), nullptr, nullptr, face.data(), closest.data());
  for (long i = 0; i < n_pts; ++i)
    if (want[i] == want[i] && !(sdf[i] > 3.0e38f && face[i] == -1 && closest[3 * i] == pts[3 * i])) return fail("n_faces = 0");
  std::vector<int32_t> none;
  for (auto& b : bad) none.insert(none.end(), b, b + 3);
  meshsdf_host_query_sliced(verts.data(), none.data(), n_verts, (int)none.size() / 3, pts.data(), n_pts, 4, sdf.data(), nullptr, nullptr, face.data(), nullptr);
  for (long i = 0; i < n_pts; ++i)
    if (want[i] == want[i] && !(sdf[i] > 3.0e38f && face[i] == -1)) return fail("all faces invalid");
  // no vertices: every index is out of range
  meshsdf_host_query(nullptr, cube.data(), 0, 12, pts.data(), n_pts, sdf.data(), nullptr, nullptr, nullptr, nullptr);
  if (!(sdf[0] > 3.0e38f)) return fail("n_verts = 0");
  // no points
  meshsdf_host_query(verts.data(), cube.data(), n_cube_verts, 12, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
  printf("meshsdf_host_main: ok, %d faces, %ld points\n", n_faces, n_pts);
  return 0;
}
