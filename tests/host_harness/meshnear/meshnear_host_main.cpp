// Stand-alone run of the grid distance query's twin (meshnear_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_meshray.h, include/lab4d_meshnear.h), so a cell read past the grid, a list read past its total or a face read past the mesh is an
// error report and a non-zero exit.  The mesh is the cube of tests/meshray_checks.py with four faces that are never listed (indices out of range, a
// NaN vertex, a degenerate face); the lists come from the ray caster's twin.  The points are a lattice through and around the box, points far
// outside it and the non-finite ones.  d2, face, closest point, region and sdf are checked against G = 1 here, the values elsewhere.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "meshnear/meshnear_host.cpp"
#include "meshray/meshray_host.cpp"

static int fail(const char* what, long r) {
  fprintf(stderr, "meshnear_host_main: %s (%ld)\n", what, r);
  return 1;
}

int main() {
  const float lo[3] = {-0.5f, -0.25f, -0.75f}, hi[3] = {0.5f, 0.75f, 0.25f}, pad = 0.0009765625f, nan = NAN, inf = INFINITY;
  std::vector<float> verts;
  for (int k = 0; k < 8; ++k) {
    const int c[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
    for (int a = 0; a < 3; ++a) verts.push_back(c[k][a] ? hi[a] : lo[a]);
  }
  verts.insert(verts.end(), {nan, 0.f, 0.f});
  const int n_verts = 9;
  std::vector<int32_t> faces = {0, 1, 99, -1, 1, 2, 0, 1, 8, 5, 5, 6,  // never listed
                                0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 3, 7, 6, 3, 6, 2, 0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5};
  const int F = (int)faces.size() / 3, n_bad = 4;
  float aabb[6];
  for (int a = 0; a < 3; ++a) aabb[a] = lo[a] - pad, aabb[3 + a] = hi[a] + pad;

  std::vector<float> pts;
  for (int i = -3; i <= 11; ++i)  // a lattice of step 1 / 8 of the extent from 3 / 8 outside to 3 / 8 outside: on the surface, on walls, inside
    for (int j = -3; j <= 11; ++j)
      for (int k = -3; k <= 11; ++k) pts.insert(pts.end(), {lo[0] + 0.125f * i, lo[1] + 0.125f * j, lo[2] + 0.125f * k});
  const float far[3] = {1.5f, 8.5f, 1024.5f};
  for (float s : far)
    for (int i = -1; i <= 1; ++i)
      for (int j = -1; j <= 1; ++j)
        for (int k = -1; k <= 1; ++k) pts.insert(pts.end(), {0.1f + s * i, 0.2f + s * j, -0.3f + s * k});
  const long n_finite = (long)pts.size() / 3;
  pts.insert(pts.end(), {nan, 0.f, 0.f, 0.f, inf, 0.f, 0.f, 0.f, -inf});
  const long N = (long)pts.size() / 3;

  std::vector<float> ref_sdf, ref_d2, ref_q;
  std::vector<int32_t> ref_face, ref_region;
  const int Gs[4] = {1, 2, 5, 32};  // (the far points walk every cell: G^3 of them each)
  for (int G : Gs) {
    float* tris = (float*)aligned_alloc(16, sizeof(float) * 12 * F);
    std::vector<int32_t> cell_start((size_t)G * G * G + 1, -7);
    const int total = meshray_host_build(verts.data(), faces.data(), n_verts, F, aabb, G, tris, cell_start.data(), nullptr);
    if (total < 12) return fail("the count lists fewer entries than the cube has faces", total);
    std::vector<int32_t> cell_list(total, -7);  // exactly the total
    if (meshray_host_build(verts.data(), faces.data(), n_verts, F, aabb, G, tris, cell_start.data(), cell_list.data()) != total)
      return fail("count and fill disagree", G);
    for (int sign_mode = 0; sign_mode <= 1; ++sign_mode) {
      std::vector<float> sdf(N, 7.f), d2(N, 7.f), q(3 * N, 7.f);
      std::vector<int32_t> face(N, -7), region(N, -7), n_tests(N, -7), n_cells(N, -7);
      if (meshnear_host_closest(pts.data(), N, tris, F, aabb, G, cell_start.data(), cell_list.data(), sign_mode, 1, sdf.data(), d2.data(), face.data(), q.data(),
                                region.data(), n_tests.data(), n_cells.data()))
        return fail("the twin refused good arguments", G);
      long inside = 0;
      for (long i = 0; i < N; ++i) {
        if (i >= n_finite) {
          if (!(isnan(sdf[i]) && isnan(d2[i]) && face[i] == -1 && region[i] == -1 && n_tests[i] == 0 && memcmp(&q[3 * i], &pts[3 * i], 12) == 0))
            return fail("a non-finite point", i);
          continue;
        }
        if (face[i] < n_bad || face[i] >= F || region[i] < 0 || region[i] > 6 || n_tests[i] < 1 || n_cells[i] < 1 || n_cells[i] > G * G * G)
          return fail("an output outside its range", i);
        if (!(d2[i] >= 0.f) || fabsf(sdf[i]) != sqrtf(d2[i]) || (sign_mode == 0 && sdf[i] < 0.f)) return fail("sdf and d2 disagree", i);
        inside += sdf[i] < 0.f;
      }
      if (sign_mode == 1 && inside != 7 * 7 * 7 + 3) return fail("343 points of the lattice and the centre of each far set lie strictly inside the cube", inside);
      if (G == 1 && sign_mode == 1) ref_sdf = sdf, ref_d2 = d2, ref_q = q, ref_face = face, ref_region = region;
      if (sign_mode == 1 && (memcmp(sdf.data(), ref_sdf.data(), 4 * N) || memcmp(d2.data(), ref_d2.data(), 4 * N) || memcmp(q.data(), ref_q.data(), 12 * N) ||
                             face != ref_face || region != ref_region))
        return fail("the result depends on G", G);
      // the optional outputs left out
      if (meshnear_host_closest(pts.data(), N, tris, F, aabb, G, cell_start.data(), cell_list.data(), sign_mode, -1, sdf.data(), nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr))
        return fail("NULL for the optional outputs must succeed", G);
    }
    free(tris);
  }
  {  // F = 0, N = 0, refused arguments
    std::vector<float> sdf(N, 7.f);
    std::vector<int32_t> face(N, -7);
    if (meshnear_host_closest(pts.data(), N, nullptr, 0, aabb, 4, nullptr, nullptr, 1, 1, sdf.data(), nullptr, face.data(), nullptr, nullptr, nullptr, nullptr))
      return fail("F = 0 must succeed", -1);
    for (long i = 0; i < n_finite; ++i)
      if (!(sdf[i] == inf && face[i] == -1)) return fail("F = 0: +inf and no face", i);
    if (meshnear_host_closest(nullptr, 0, nullptr, 0, aabb, 4, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
      return fail("N = 0 must succeed", -1);
    if (meshnear_host_closest(pts.data(), N, nullptr, 0, aabb, 129, nullptr, nullptr, 1, 1, sdf.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != -1)
      return fail("G = 129 must be refused", -1);
    if (meshnear_host_closest(pts.data(), N, nullptr, 0, aabb, 4, nullptr, nullptr, 2, 1, sdf.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != -1)
      return fail("sign_mode = 2 must be refused", -1);
    if (meshnear_host_closest(pts.data(), N, nullptr, 0, aabb, 4, nullptr, nullptr, 1, 0, sdf.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != -1)
      return fail("orient = 0 must be refused", -1);
  }
  printf("meshnear_host_main: ok, %ld points\n", N);
  return 0;
}
