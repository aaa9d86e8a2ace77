// Stand-alone run of the mesh ray caster's twin (meshray_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_meshray.h), so a list written past its total, a cell read past the grid or a face read past the mesh is an error report and a
// non-zero exit.  The mesh is the cube of tests/meshray_checks.py with five faces that must never be listed (indices out of range, a NaN
// vertex, a degenerate face, a face outside the box); the rays are the degenerate ones of the rules plus a fan through the box.  The hits are
// checked against G = 1 here, the values elsewhere.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "meshray/meshray_host.cpp"

static int fail(const char* what, long r) {
  fprintf(stderr, "meshray_host_main: %s (%ld)\n", what, r);
  return 1;
}

struct Grid {
  float* tris;  // 16-byte aligned, exactly 12 * F floats
  std::vector<int32_t> cell_start, cell_list;
};

int main() {
  const float lo[3] = {-0.5f, -0.25f, -0.75f}, hi[3] = {0.5f, 0.75f, 0.25f}, pad = 0.0009765625f, nan = NAN, inf = INFINITY;
  std::vector<float> verts;
  for (int k = 0; k < 8; ++k) {
    const int c[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
    for (int a = 0; a < 3; ++a) verts.push_back(c[k][a] ? hi[a] : lo[a]);
  }
  const float extra[4][3] = {{nan, 0.f, 0.f}, {2.f, 2.f, 2.f}, {2.5f, 2.f, 2.f}, {2.f, 2.5f, 2.f}};
  for (const auto& e : extra) verts.insert(verts.end(), e, e + 3);
  const int n_verts = 12;
  std::vector<int32_t> faces = {0, 1, 99, -1, 1, 2, 0, 1, 8, 5, 5, 6, 9, 10, 11,  // never listed
                                0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 3, 7, 6, 3, 6, 2, 0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5};
  const int F = (int)faces.size() / 3;
  float aabb[6];
  for (int a = 0; a < 3; ++a) aabb[a] = lo[a] - pad, aabb[3 + a] = hi[a] + pad;

  struct Ray { float o[3], d[3], t0, t1; };
  std::vector<Ray> rays = {
      {{0.f, 0.25f, -2.f}, {0.f, 0.f, 1.f}, 0.f, 4.f},       {{2.f, 0.375f, -0.125f}, {-2.f, 0.f, 0.f}, 0.f, 4.f}, {{-2.f, 0.375f, -0.125f}, {-1.f, 0.f, 0.f}, -4.f, 0.f},
      {{0.125f, 0.5f, -2.f}, {0.f, 0.f, 0.f}, 0.f, 4.f},     {{0.125f, 0.5f, -2.f}, {0.f, 0.f, 1e-30f}, 0.f, 4.f}, {{nan, 0.5f, -2.f}, {0.f, 0.f, 1.f}, 0.f, 4.f},
      {{0.125f, inf, -2.f}, {0.f, 0.f, 1.f}, 0.f, 4.f},      {{0.125f, 0.5f, -2.f}, {nan, 0.f, 1.f}, 0.f, 4.f},    {{0.125f, 0.5f, -2.f}, {0.f, 0.f, -inf}, 0.f, 4.f},
      {{0.125f, 0.5f, -2.f}, {0.f, 0.f, 1.f}, nan, 4.f},     {{0.125f, 0.5f, -2.f}, {0.f, 0.f, 1.f}, 0.f, inf},    {{0.125f, 0.5f, -2.f}, {0.f, 0.f, 1.f}, 3.f, 2.f},
      {{0.125f, 0.5f, -2.f}, {0.f, 0.f, 1.f}, 1.25f, 1.25f}, {{0.125f, 0.5f, -2.f}, {0.f, 0.f, 1.f}, 1.5f, 1.5f},  {{0.125f, 0.5f, -2.f}, {0.f, 0.f, 1.f}, 1.f, 1.f},
      {{0.f, 0.5f, -2.f}, {0.f, 0.f, 1.f}, 0.f, 4.f},        {{-2.f, -1.75f, -2.25f}, {1.f, 1.f, 1.f}, 0.f, 4.f},  {{3.f, 0.5f, -2.f}, {0.f, 0.f, 1.f}, 0.f, 4.f},
      {{0.f, 0.25f, -2.f}, {0.3f, 0.3f, -1.f}, 0.f, 4.f},    {{0.125f, 0.5f, -0.25f}, {1.f, 0.f, 0.f}, 0.f, 4.f},  {{2.2f, 2.2f, 0.f}, {0.f, 0.f, 1.f}, 0.f, 4.f},
  };
  for (int i = 0; i < 17; ++i)  // a fan from one corner region through the box, some rays missing the cube
    for (int j = 0; j < 17; ++j) rays.push_back({{-2.f, -2.f, -2.5f}, {1.f + 0.11f * i, 1.2f + 0.09f * j, 1.3f}, 0.f, 6.f});
  const long R = (long)rays.size();
  std::vector<float> origin(3 * R), dir(3 * R), t_range(2 * R);
  for (long r = 0; r < R; ++r) {
    for (int a = 0; a < 3; ++a) origin[3 * r + a] = rays[r].o[a], dir[3 * r + a] = rays[r].d[a];
    t_range[2 * r] = rays[r].t0, t_range[2 * r + 1] = rays[r].t1;
  }

  std::vector<float> t_ref;
  std::vector<int32_t> face_ref;
  const int Gs[4] = {1, 2, 5, 128};
  for (int G : Gs) {
    Grid g;
    g.tris = (float*)aligned_alloc(16, sizeof(float) * 12 * F);
    g.cell_start.assign((size_t)G * G * G + 1, -7);
    const int total = meshray_host_build(verts.data(), faces.data(), n_verts, F, aabb, G, g.tris, g.cell_start.data(), nullptr);
    if (total < 12) return fail("the count lists fewer entries than the cube has faces", total);
    g.cell_list.assign(total, -7);  // exactly the total: one entry more is a heap overflow
    if (meshray_host_build(verts.data(), faces.data(), n_verts, F, aabb, G, g.tris, g.cell_start.data(), g.cell_list.data()) != total)
      return fail("count and fill disagree", G);
    for (int32_t f : g.cell_list)
      if (f < 5 || f >= F) return fail("a face that must not be listed is", f);
    std::vector<float> t(R, 7.f), u(R, 7.f), v(R, 7.f);
    std::vector<int32_t> face(R, -7), front(R, -7), n_tests(R, -7);
    if (meshray_host_cast(origin.data(), dir.data(), t_range.data(), R, g.tris, F, aabb, G, g.cell_start.data(), g.cell_list.data(), t.data(), face.data(),
                          u.data(), v.data(), front.data(), n_tests.data()))
      return fail("the twin refused good arguments", G);
    long hits = 0;
    for (long r = 0; r < R; ++r) {
      if (face[r] < -1 || face[r] >= F || (face[r] >= 0 && face[r] < 5) || n_tests[r] < 0 || front[r] < 0 || front[r] > 1) return fail("an output outside its range", r);
      if (face[r] < 0 && !(u[r] == 0.f && v[r] == 0.f && front[r] == 0 && (t[r] == rays[r].t0 || (isnan(t[r]) && isnan(rays[r].t0))))) return fail("a miss", r);
      if (face[r] >= 0 && !(t[r] >= rays[r].t0 && t[r] <= rays[r].t1 && u[r] >= 0.f && v[r] >= 0.f)) return fail("a hit outside its range", r);
      hits += face[r] >= 0;
    }
    if (hits < 50) return fail("too few hits", hits);
    if (G == 1) t_ref = t, face_ref = face;
    else if (memcmp(t.data(), t_ref.data(), sizeof(float) * R) || face != face_ref) return fail("the result depends on G", G);
    free(g.tris);
  }
  // F = 0 and R = 0: nothing is read or written
  if (meshray_host_cast(nullptr, nullptr, nullptr, 0, nullptr, 0, aabb, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
    return fail("R = 0 must succeed", -1);
  {
    std::vector<float> t(R), u(R), v(R);
    std::vector<int32_t> face(R), front(R), n_tests(R);
    if (meshray_host_cast(origin.data(), dir.data(), t_range.data(), R, nullptr, 0, aabb, 4, nullptr, nullptr, t.data(), face.data(), u.data(), v.data(),
                          front.data(), n_tests.data()))
      return fail("F = 0 must succeed", -1);
    for (long r = 0; r < R; ++r)
      if (face[r] != -1 || n_tests[r] != 0) return fail("F = 0: every ray misses without a test", r);
  }
  if (meshray_host_build(verts.data(), faces.data(), n_verts, F, aabb, 129, nullptr, nullptr, nullptr) != -1) return fail("G = 129 must be refused", -1);
  printf("meshray_host_main: ok, %ld rays\n", R);
  return 0;
}
